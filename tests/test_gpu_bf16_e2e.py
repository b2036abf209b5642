"""A BF16 GGUF end to end through the reference's libllama (oracle/_ref/llama-e2e, tests/cpp/llama_e2e.cpp): the tiny llama model written
by tests/gguf_synth.py (2 layers, n_embd 1024, n_ff 2816, 8 / 2 heads, vocab 4096; matmul weights and token_embd BF16) is loaded by
llama_model_load_from_file, its matmul weights land in the device's buffer and the logits are compared with the ggml CPU backend.
Ceiling: the project's end-to-end bar, worst NMSE < 5e-3 (test_gpu_llama_e2e.py); the measured values are printed.  Before BF16 was
a weight type of the device every matmul weight of such a file stayed in a CPU buffer."""
import json
import os
import subprocess
from pathlib import Path

import pytest

import gguf_synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
E2E = ROOT / "oracle" / "_ref" / "llama-e2e"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"


def run(*args, env=None, timeout=600):
    if not E2E.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/llama-e2e or the plugin module is not built (needs the reference tree at build time)")
    e = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), **(env or {}))
    p = subprocess.run([str(E2E), *args], env=e, capture_output=True, text=True, timeout=timeout, cwd=str(E2E.parent))
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1]) if lines else None


@pytest.fixture(scope="module")
def gguf(tmp_path_factory):
    if not E2E.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/llama-e2e or the plugin module is not built (needs the reference tree at build time)")
    return str(gguf_synth.write_tiny_llama_bf16(tmp_path_factory.mktemp("gguf") / "tiny-bf16.gguf"))


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_logits_match_cpu_backend_matvec_path(gguf, fuse):
    r = run("compare", "--gguf", gguf, "-p", "8", "-n", "8", "-t", "8", env={"GGML_MI355X_FUSE": fuse})
    print(r)
    assert "MI355X0" in r["devices"]
    assert r["worst_nmse"] < 5e-3, r


def test_logits_match_cpu_backend_prefill_path(gguf):
    r = run("compare", "--gguf", gguf, "-p", "64", "-n", "8", "-t", "8")
    print(r)
    assert r["worst_nmse"] < 5e-3, r


def test_row_split_over_two_logical_devices(gguf):
    r = run("compare", "--gguf", gguf, "-p", "40", "-n", "4", "-t", "8", "-sm", "row", env={"GGML_MI355X_VIRTUAL_DEVICES": "2"})
    print(r)
    assert r["worst_nmse"] < 5e-3, r


def test_partial_offload(gguf):
    r = run("compare", "--gguf", gguf, "-p", "40", "-n", "4", "-t", "8", "--ngl", "1")
    print(r)
    assert r["worst_nmse"] < 5e-3, r


def test_matmul_weights_live_in_the_device_buffer(gguf):
    r = run("bench", "--gguf", gguf, "-p", "128", "-n", "16", "-r", "1", "-t", "8")
    print(r)
    assert r["pp_tok_s"] > 0 and r["tg_tok_s"] > 0
    # 51 MiB of matmul weights (2 layers of 21.5 MiB and the 8 MiB output matrix) on the device; the 8 MiB input embedding (BF16
    # GET_ROWS is out of scope) stays with the host
    buf = r["model_buffers_MiB"]
    dev_mib = sum(v for k, v in buf.items() if "MI355X" in k)
    cpu_mib = sum(v for k, v in buf.items() if "MI355X" not in k)
    assert dev_mib > 40 and cpu_mib < 10, buf
