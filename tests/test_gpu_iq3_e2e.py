"""A 3-bit i-quant GGUF end to end through the reference's libllama (oracle/_ref/llama-e2e, tests/cpp/llama_e2e.cpp): the tiny llama model
of tests/iq3_gguf.py (2 layers, n_embd 1024, n_ff 2816, 8 / 2 heads, vocab 4096; tensor types as a stock IQ3_XXS file has them, quantized
by the reference's own quantizer) is loaded by llama_model_load_from_file; the plugin derives the two grids from ggml, the matmul weights
land in the device's buffer and the logits are compared with the ggml CPU backend.  Ceiling: the project's end-to-end bar, worst NMSE <
5e-3 (test_gpu_llama_e2e.py); the measured values are printed.  Before IQ3_XXS / IQ3_S were weight types of the device the IQ3 tensors
of such a file stayed in a CPU buffer."""
import json
import os
import subprocess
from pathlib import Path

import pytest

import iq3_gguf
import iq3_refs

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
def model(tmp_path_factory):
    if not E2E.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/llama-e2e or the plugin module is not built (needs the reference tree at build time)")
    path, sizes = iq3_gguf.write_tiny_llama_iq3(tmp_path_factory.mktemp("gguf") / "tiny-iq3_xxs.gguf", iq3_refs.Iq3Ref())
    return str(path), sizes


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_logits_match_cpu_backend_matvec_path(model, fuse):
    r = run("compare", "--gguf", model[0], "-p", "8", "-n", "8", "-t", "8", env={"GGML_MI355X_FUSE": fuse})
    print(r)
    assert "MI355X0" in r["devices"]
    assert r["worst_nmse"] < 5e-3, r


def test_logits_match_cpu_backend_prefill_path(model):
    r = run("compare", "--gguf", model[0], "-p", "64", "-n", "8", "-t", "8")
    print(r)
    assert r["worst_nmse"] < 5e-3, r


def test_row_split_over_two_logical_devices(model):
    r = run("compare", "--gguf", model[0], "-p", "40", "-n", "4", "-t", "8", "-sm", "row", env={"GGML_MI355X_VIRTUAL_DEVICES": "2"})
    print(r)
    assert r["worst_nmse"] < 5e-3, r


def test_partial_offload(model):
    r = run("compare", "--gguf", model[0], "-p", "40", "-n", "4", "-t", "8", "--ngl", "1")
    print(r)
    assert r["worst_nmse"] < 5e-3, r


def test_matmul_weights_live_in_the_device_buffer(model):
    path, sizes = model
    r = run("bench", "--gguf", path, "-p", "128", "-n", "16", "-r", "1", "-t", "8")
    print(r)
    assert r["pp_tok_s"] > 0 and r["tg_tok_s"] > 0
    # every matmul weight on the device; the input embedding (llama.cpp keeps it with the host) and nothing else of them on the CPU
    MiB = 1024.0 * 1024.0
    matmul = sum(v for k, v in sizes.items() if k != "token_embd.weight") / MiB
    iq3 = sum(v for k, v in sizes.items() if k != "token_embd.weight" and "attn_v" not in k and k != "output.weight") / MiB
    buf = r["model_buffers_MiB"]
    on_dev = lambda name: "MI355X" in name and "Host" not in name           # (MI355X_Host: the pinned host buffer type)
    dev_mib = sum(v for k, v in buf.items() if on_dev(k))
    cpu_mib = sum(v for k, v in buf.items() if not on_dev(k))
    print(f"matmul weights {matmul:.2f} MiB (IQ3: {iq3:.2f}), token_embd {sizes['token_embd.weight'] / MiB:.2f} MiB; device {dev_mib:.2f}, host {cpu_mib:.2f}")
    # without the two types the device would hold matmul - iq3 (attn_v and output only)
    assert dev_mib >= matmul - 0.1 and cpu_mib <= sizes["token_embd.weight"] / MiB + 0.5, buf
