"""GGUFs in the stock TQ1_0 / TQ2_0 layouts end to end through the reference's libllama (oracle/_ref/llama-e2e,
tests/cpp/llama_e2e.cpp): the two tiny models of tests/tq_gguf.py.  "tq2_0" is a dense file (every matmul tensor TQ2_0 but a Q6_K
output), "tq1_0_moe" an 8-expert one (attn_k / attn_v Q8_0, everything else TQ1_0).  llama_model_load_from_file loads them, every
matmul weight lands in the device's buffers, and the logits are compared with the ggml CPU backend.
Ceiling: the project's end-to-end bar, worst NMSE < 5e-3 (test_gpu_llama_e2e.py); the measured values are printed.  Before TQ1_0 /
TQ2_0 were weight types of the device, such a file kept everything but `output` (and the MoE file's attn_k / attn_v) in a CPU buffer
and the two placement tests fail."""
import json
import os
import subprocess
from pathlib import Path

import pytest

import tq_gguf
import tq_refs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
E2E = ROOT / "oracle" / "_ref" / "llama-e2e"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"
KINDS = ["tq1_0_moe", "tq2_0"]
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
    ref, d = tq_refs.TqRef(), tmp_path_factory.mktemp("gguf")
    out = {}
    for kind in KINDS:
        path, sizes = tq_gguf.write_tiny_llama(kind, d / f"tiny-{kind}.gguf", ref)
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
def test_every_matmul_weight_sits_in_the_device_buffers(models, kind):
    path, sizes = models[kind]
    r = run("bench", "--gguf", path, "-p", "128", "-n", "16", "-r", "1", "-t", "8")
    print(kind, r)
    assert r["pp_tok_s"] > 0 and r["tg_tok_s"] > 0
    embd = sizes["token_embd.weight"] / MiB
    matmul = sum(v for k, v in sizes.items() if k != "token_embd.weight") / MiB
    tq = sum(sizes[name] for name, typ, *_ in tq_gguf.layout(kind) if typ in (tq_gguf.TQ1_0, tq_gguf.TQ2_0)) / MiB
    buf = r["model_buffers_MiB"]
    on_dev = lambda name: "MI355X" in name and "Host" not in name              # (MI355X_Host: the pinned host buffer type)
    dev_mib = sum(v for k, v in buf.items() if on_dev(k))
    cpu_mib = sum(v for k, v in buf.items() if not on_dev(k))
    print(f"{kind}: matmul weights {matmul:.2f} MiB (TQ: {tq:.2f}), token_embd {embd:.2f} MiB; device {dev_mib:.2f}, host {cpu_mib:.2f}")
    # every matmul weight on the device; the input embedding (llama.cpp keeps it with the host) and nothing else of them on the CPU.
    # Without the two types the device would hold matmul - tq, and the host the rest
    assert tq > 0.6
    assert dev_mib >= matmul - 0.1 and cpu_mib <= embd + 0.5, buf
