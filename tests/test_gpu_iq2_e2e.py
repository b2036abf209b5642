"""GGUFs that hold IQ2_XS / IQ2_S tensors end to end through the reference's libllama (oracle/_ref/llama-e2e, tests/cpp/llama_e2e.cpp):
the tiny llama model of tests/iq2_gguf.py (2 layers, n_embd 1024, n_ff 2816, 8 / 2 heads, vocab 4096) in the two stock layouts read off
llama-quant.cpp there: what a real IQ3_XXS file holds (attn_q / attn_k IQ2_S beside IQ3_XXS, IQ3_S, Q4_K, Q5_K) and an IQ2_XS file (IQ2_XS
beside Q4_K, Q5_K and a Q2_K token_embd), quantized by the reference's own quantizer.  llama_model_load_from_file loads them; the plugin
derives the grids from ggml, the matmul weights land in the device's buffer and the logits are compared with the ggml CPU backend.
Ceiling: the project's end-to-end bar, worst NMSE < 5e-3 (test_gpu_llama_e2e.py); the measured values are printed.  Before IQ2_XS / IQ2_S
were weight types of the device, the IQ2 tensors of such files stayed in a CPU buffer and the last test fails."""
import json
import os
import subprocess
from pathlib import Path

import pytest

import iq2_gguf
import iq2_refs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
E2E = ROOT / "oracle" / "_ref" / "llama-e2e"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"
KINDS = ["iq3_xxs", "iq2_xs"]


def run(*args, env=None, timeout=600):
    if not E2E.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/llama-e2e or the plugin module is not built (needs the reference tree at build time)")
    e = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), **(env or {}))
    p = subprocess.run([str(E2E), *args], env=e, capture_output=True, text=True, timeout=timeout, cwd=str(E2E.parent))
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1]) if lines else None


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    if not E2E.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/llama-e2e or the plugin module is not built (needs the reference tree at build time)")
    ref, d = iq2_refs.Iq2Ref(), tmp_path_factory.mktemp("gguf")
    out = {}
    for kind in KINDS:
        path, sizes = iq2_gguf.write_tiny_llama(kind, d / f"tiny-{kind}.gguf", ref)
        out[kind] = (str(path), sizes)
    return out


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("kind", KINDS)
def test_logits_match_cpu_backend_matvec_path(models, kind, fuse):
    r = run("compare", "--gguf", models[kind][0], "-p", "8", "-n", "8", "-t", "8", env={"GGML_MI355X_FUSE": fuse})
    print(kind, r)
    assert "MI355X0" in r["devices"]
    assert r["worst_nmse"] < 5e-3, r


@pytest.mark.parametrize("kind", KINDS)
def test_logits_match_cpu_backend_prefill_path(models, kind):
    r = run("compare", "--gguf", models[kind][0], "-p", "64", "-n", "8", "-t", "8")
    print(kind, r)
    assert r["worst_nmse"] < 5e-3, r


@pytest.mark.parametrize("kind", KINDS)
def test_row_split_over_two_logical_devices(models, kind):
    r = run("compare", "--gguf", models[kind][0], "-p", "40", "-n", "4", "-t", "8", "-sm", "row", env={"GGML_MI355X_VIRTUAL_DEVICES": "2"})
    print(kind, r)
    assert r["worst_nmse"] < 5e-3, r


@pytest.mark.parametrize("kind", KINDS)
def test_partial_offload(models, kind):
    r = run("compare", "--gguf", models[kind][0], "-p", "40", "-n", "4", "-t", "8", "--ngl", "1")
    print(kind, r)
    assert r["worst_nmse"] < 5e-3, r


@pytest.mark.parametrize("kind", KINDS)
def test_matmul_weights_live_in_the_device_buffer(models, kind):
    path, sizes = models[kind]
    r = run("bench", "--gguf", path, "-p", "128", "-n", "16", "-r", "1", "-t", "8")
    print(kind, r)
    assert r["pp_tok_s"] > 0 and r["tg_tok_s"] > 0
    # every matmul weight on the device; the input embedding (llama.cpp keeps it with the host) and nothing else of them on the CPU
    MiB = 1024.0 * 1024.0
    iq2_types = (iq2_gguf.IQ2_XS, iq2_gguf.IQ2_S)
    matmul = sum(v for k, v in sizes.items() if k != "token_embd.weight") / MiB
    iq2 = sum(sizes[name] for name, typ, _, _ in iq2_gguf.layout(kind) if typ in iq2_types and name != "token_embd.weight") / MiB
    buf = r["model_buffers_MiB"]
    on_dev = lambda name: "MI355X" in name and "Host" not in name           # (MI355X_Host: the pinned host buffer type)
    dev_mib = sum(v for k, v in buf.items() if on_dev(k))
    cpu_mib = sum(v for k, v in buf.items() if not on_dev(k))
    print(f"{kind}: matmul weights {matmul:.2f} MiB (IQ2: {iq2:.2f}), token_embd {sizes['token_embd.weight'] / MiB:.2f} MiB; device {dev_mib:.2f}, host {cpu_mib:.2f}")
    # without the two types the device would hold matmul - iq2, and the host the rest
    assert iq2 > 0.6
    assert dev_mib >= matmul - 0.1 and cpu_mib <= sizes["token_embd.weight"] / MiB + 0.5, buf
