"""GGUFs that hold IQ1_S / IQ1_M tensors end to end through the reference's libllama (oracle/_ref/llama-e2e, tests/cpp/llama_e2e.cpp):
the two tiny models of tests/iq1_gguf.py in the stock layouts read off llama-quant.cpp there.  "iq1_m_moe" is what an 8-expert IQ1_M
download holds (attn_q and the three expert tensors IQ1_M beside Q4_K, Q5_K and a Q2_K token_embd); "iq1_s" is a dense IQ1_S file, whose
attn_output is IQ2_XXS, a type the device does not run.  llama_model_load_from_file loads them; the plugin derives the grid from ggml,
the matmul weights it can run land in the device's buffer and the logits are compared with the ggml CPU backend.
Ceiling: the project's end-to-end bar, worst NMSE < 5e-3 (test_gpu_llama_e2e.py); the measured values are printed.  Before IQ1_S / IQ1_M
were weight types of the device, the IQ1 tensors of such files stayed in a CPU buffer and the two placement tests fail."""
import json
import os
import subprocess
from pathlib import Path

import pytest

import iq1_gguf
import iq1_refs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
E2E = ROOT / "oracle" / "_ref" / "llama-e2e"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"
KINDS = ["iq1_m_moe", "iq1_s"]
MiB = 1024.0 * 1024.0


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
    ref, d = iq1_refs.Iq1Ref(), tmp_path_factory.mktemp("gguf")
    out = {}
    for kind in KINDS:
        path, sizes = iq1_gguf.write_tiny_llama(kind, d / f"tiny-{kind}.gguf", ref)
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


def placement(models, kind):
    """(bytes by tensor, MiB in the device's buffers, MiB elsewhere, MiB of IQ1 matmul tensors, MiB of all matmul tensors)"""
    path, sizes = models[kind]
    r = run("bench", "--gguf", path, "-p", "128", "-n", "16", "-r", "1", "-t", "8")
    print(kind, r)
    assert r["pp_tok_s"] > 0 and r["tg_tok_s"] > 0
    matmul = sum(v for k, v in sizes.items() if k != "token_embd.weight") / MiB
    iq1 = sum(sizes[name] for name, typ, *_ in iq1_gguf.layout(kind) if typ in (iq1_gguf.IQ1_S, iq1_gguf.IQ1_M)) / MiB
    buf = r["model_buffers_MiB"]
    on_dev = lambda name: "MI355X" in name and "Host" not in name              # (MI355X_Host: the pinned host buffer type)
    dev_mib = sum(v for k, v in buf.items() if on_dev(k))
    cpu_mib = sum(v for k, v in buf.items() if not on_dev(k))
    return sizes, dev_mib, cpu_mib, iq1, matmul, buf


def test_moe_iq1_m_file_keeps_every_matmul_weight_in_the_device_buffer(models):
    sizes, dev_mib, cpu_mib, iq1, matmul, buf = placement(models, "iq1_m_moe")
    embd = sizes["token_embd.weight"] / MiB
    print(f"iq1_m_moe: matmul weights {matmul:.2f} MiB (IQ1: {iq1:.2f}), token_embd {embd:.2f} MiB; device {dev_mib:.2f}, host {cpu_mib:.2f}")
    # every matmul weight on the device; the input embedding (llama.cpp keeps it with the host) and nothing else of them on the CPU.
    # Without the two types the device would hold matmul - iq1, and the host the rest
    assert iq1 > 0.6
    assert dev_mib >= matmul - 0.1 and cpu_mib <= embd + 0.5, buf


def test_dense_iq1_s_file_keeps_only_the_iq2_xxs_tensors_on_the_host(models):
    sizes, dev_mib, cpu_mib, iq1, matmul, buf = placement(models, "iq1_s")
    embd = sizes["token_embd.weight"] / MiB
    xxs = sum(sizes[name] for name, typ, *_ in iq1_gguf.layout("iq1_s") if typ == iq1_gguf.IQ2_XXS) / MiB
    print(f"iq1_s: matmul weights {matmul:.2f} MiB (IQ1: {iq1:.2f}, IQ2_XXS attn_output: {xxs:.2f}), token_embd {embd:.2f} MiB; device {dev_mib:.2f}, host {cpu_mib:.2f}")
    assert iq1 > 0.6
    assert cpu_mib <= embd + xxs + 0.5 and dev_mib >= matmul - xxs - 0.1, buf
