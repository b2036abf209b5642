"""GGML_OP_FLASH_ATTN_EXT through the plugin, judged by the REFERENCE's own parity harness (tests/test-backend-ops.cpp, built unmodified
into oracle/_ref): every case of the supported surface (F16 K / V, an f16 mask, no ALiBi, no soft-cap, head sizes 64 and 128) is compared
with the ggml CPU backend (NMSE <= 5e-4, tests/test-backend-ops.cpp:3240) and none of them may be reported as not supported; everything
outside that surface is refused, never computed wrongly."""
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TBO = ROOT / "oracle" / "_ref" / "test-backend-ops"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"

# the harness filters on vars() (tests/test-backend-ops.cpp:3236):
#   hsk=128,hsv=128,nh=4,nr=1,kv=512,nb=1,mask=1,max_bias=0.000000,logit_softcap=0.000000,prec=f32,type_KV=f16,permute=[0,1,2,3]
SURFACE = r"hsk=(64|128),hsv=(64|128),nh=\d+,nr=\d+,kv=\d+,nb=\d+,mask=1,max_bias=0\.000000,logit_softcap=0\.000000,prec=(f32|def),type_KV=f16,permute="
# its loops (:4417-4449) with those values: per nb in {1, 3, 32, 35}, head size 64 (prec f32 only): (nr, kv) = (1, 512), (4, 512) plain and
# permuted, (1, 1024) plain = 5; head size 128: the same and (16, 512) plain and permuted = 7, for both prec values: 4 * (5 + 2 * 7)
SURFACE_CASES = 76


def run_tbo(*args, timeout=900):
    if not TBO.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/test-backend-ops or the plugin module is not built (needs the reference tree at build time)")
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    p = subprocess.run([str(TBO), *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(TBO.parent))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)


def summarize(out):
    ok = len(re.findall(r"\): OK", out))
    fail = [l for l in out.splitlines() if "FAIL" in l or "ERR =" in l]
    unsup = len(re.findall(r"not supported \[", out))
    return ok, fail, unsup


def test_reference_harness_passes_the_flash_attention_surface():
    rc, out = run_tbo("test", "-o", "FLASH_ATTN_EXT", "-p", SURFACE)
    assert "MI355X0" in out, out[-2000:]
    ok, fail, unsup = summarize(out)
    print(f"FLASH_ATTN_EXT, supported surface: {ok} OK, {len(fail)} failed, {unsup} not supported")
    assert not fail, "\n".join(fail[:20])
    assert rc == 0, out[-3000:]
    assert unsup == 0, out[-3000:]
    assert ok == SURFACE_CASES, (ok, out[-2000:])


def test_reference_harness_sees_no_wrong_flash_attention_result_anywhere():
    """the whole op: what is outside the surface (no mask, ALiBi, soft-cap, head sizes 80 / 192 / 256, BF16 / Q8_0 / Q4_0 caches) is reported
    as not supported; the OK count is the surface's"""
    rc, out = run_tbo("test", "-o", "FLASH_ATTN_EXT")
    ok, fail, unsup = summarize(out)
    print(f"FLASH_ATTN_EXT, every case: {ok} OK, {len(fail)} failed, {unsup} not supported")
    assert not fail, "\n".join(fail[:20])
    assert rc == 0, out[-3000:]
    assert ok == SURFACE_CASES and unsup > 0, (ok, unsup)
