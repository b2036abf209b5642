"""QMM_PREC_Q8_EXACT on Q2_K, Q3_K and IQ4_XS weights: mfma_q8x_kernel<10 | 11 | 23> (csrc/qmm_mfma_q8x.hiph) forms the integers of
ggml_vec_dot_{q2_K,q3_K,iq4_xs}_q8_K on the int8 MFMA and converts them to f32 once per 256-weight superblock.

Bar: the project's bar for "only the f32 summation order differs from the CPU backend", max |err| / rms(want) <= 2e-5 (test_gpu_parity.py,
test_gpu_q8_exact.py); `want` is always the CPU oracle on ACT_REF activations.  tests/test_q8_exact_more_host.py shows on the same inputs
(tests/q8x_refs.py) that the kernel's arithmetic, restated in numpy, is inside it.  While the mode covered Q4_K / Q5_K / Q6_K only, these
calls ran the default mode's f16 kernels in q8 mode, near 2e-3: the parity, trace and q8_exact_supported tests fail there."""
import json
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ggml_hexagon_amd.synth as synth  # noqa: E402
import gguf_synth  # noqa: E402
import q8x_refs  # noqa: E402
from oracle.pyoracle import ACT_REF, IQ4_XS, Q2_K, Q3_K, Q4_0, Q4_K, Q6_K, TYPE_NAMES  # noqa: E402
from q8x_refs import BAR, IDS, MORE, rel_rms, uniform  # noqa: E402

PREC_F16_Q8, PREC_Q8_EXACT = 1, 2


@pytest.fixture(scope="module")
def qmm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    yield q
    q.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def exact(qmm, fn):
    """fn() in the exact mode; the context is back in the default mode afterwards, whatever happens"""
    qmm.set_precision(PREC_Q8_EXACT)
    try:
        return fn()
    finally:
        qmm.set_precision(PREC_F16_Q8)


def exact_err(qmm, oracle, t, w, k, x):
    got = exact(qmm, lambda: qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy())
    return rel_rms(got, oracle.mul_mat(t, w, k, x, ACT_REF))


# ----------------------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("t", MORE, ids=IDS)
@pytest.mark.parametrize("n", q8x_refs.GRID_N)
def test_parity_grid(qmm, oracle, t, n):
    err = exact_err(qmm, oracle, t, *q8x_refs.grid_case(t, n))
    print(TYPE_NAMES[t], n, err)
    assert err <= BAR, err


@pytest.mark.parametrize("t", MORE, ids=IDS)
@pytest.mark.parametrize("m,k,n", q8x_refs.RAGGED)
def test_ragged_and_edge_shapes(qmm, oracle, t, m, k, n):
    err = exact_err(qmm, oracle, t, *q8x_refs.ragged_case(t, m, k, n))
    print(TYPE_NAMES[t], (m, k, n), err)
    assert err <= BAR, err


@pytest.mark.parametrize("t", MORE, ids=IDS)
def test_strided_destination_and_padded_weight_rows(qmm, oracle, t):
    w, k, x = q8x_refs.strided_case(t)
    m, n = w.shape[0], x.shape[0]
    want = oracle.mul_mat(t, w, k, x, ACT_REF)
    big = torch.full((n, m + 8), 3.0, device="cuda")
    exact(qmm, lambda: qmm.mul_mat(t, dev(w), k, dev(x), out=big[:, :m]))
    assert (big[:, m:] == 3.0).all()
    err = rel_rms(big[:, :m].cpu().numpy(), want)
    # weight rows further apart than the packed row (w_row_bytes = w.stride(0)); the spare bytes hold 0xFF
    wide = torch.full((m, w.shape[1] + 6), 0xFF, dtype=torch.uint8, device="cuda")
    wide[:, :w.shape[1]] = dev(w)
    got = exact(qmm, lambda: qmm.mul_mat(t, wide[:, :w.shape[1]], k, dev(x)).cpu().numpy())
    print(TYPE_NAMES[t], "strided dst", err, "padded rows", rel_rms(got, want))
    assert err <= BAR and rel_rms(got, want) <= BAR


# ----------------------------------------------------------------------------- 2. integer range edges

@pytest.mark.parametrize("name", list(q8x_refs.EDGES))
def test_range_edges(qmm, oracle, name):
    """crafted blocks (q8x_refs.EDGES: every weight of the matrix holds the named v = sc * q) against whole rows of q8 at +127 / -127"""
    t, w, k, x = q8x_refs.edge_case(name)
    want = oracle.mul_mat(t, w, k, x, ACT_REF)
    got = exact(qmm, lambda: qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy())
    print(name, "rms", float(np.sqrt(np.mean(want.astype(np.float64) ** 2))), rel_rms(got, want))
    assert rel_rms(got, want) <= BAR


# ----------------------------------------------------------------------------- 3. beyond the f16 range

@pytest.mark.parametrize("t", MORE, ids=IDS)
def test_block_beyond_the_f16_range_is_exact_and_raises_nothing(qmm, oracle, t):
    """one block with d = 65504 (Q2_K: dmin too): integers have no such range, and nothing is reported at synchronize"""
    w, k, x = q8x_refs.f16_top_case(t)
    want = oracle.mul_mat(t, w, k, x, ACT_REF)
    assert np.isfinite(want).all()
    qmm.synchronize()

    def run():
        got = qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy()
        qmm.synchronize()                                        # raises on a reported overflow
        return got
    err = rel_rms(exact(qmm, run), want)
    print(TYPE_NAMES[t], err)
    assert err <= BAR


# ----------------------------------------------------------------------------- 4. determinism and mode isolation

@pytest.mark.parametrize("t", MORE, ids=IDS)
def test_deterministic_and_leaves_the_other_paths_alone(qmm, t):
    k, m, n = 1024, 200, 130
    w, x = dev(synth.synth_weights(t, m, k, seed=1, sigma=0.3)), dev(uniform(2, n, k))
    before = qmm.mul_mat(t, w, k, x)
    few = qmm.mul_mat(t, w, k, x[:4])
    a = exact(qmm, lambda: qmm.mul_mat(t, w, k, x))
    b, few_exact = exact(qmm, lambda: (qmm.mul_mat(t, w, k, x), qmm.mul_mat(t, w, k, x[:4])))
    assert torch.equal(a, b)
    assert not torch.equal(a, before)                            # it is another computation
    assert torch.equal(qmm.mul_mat(t, w, k, x), before)
    assert torch.equal(few, few_exact)                           # the mat-vec path has no modes


# ----------------------------------------------------------------------------- 5. the plan is visible

@pytest.mark.parametrize("t", MORE, ids=IDS)
def test_trace_names_the_exact_kernel(qmm, t):
    k, m, n = 1024, 200, 64
    w, x = dev(synth.synth_weights(t, m, k, seed=1, sigma=0.3)), dev(uniform(2, n, k))
    labels = exact(qmm, lambda: qmm.trace(lambda: qmm.mul_mat(t, w, k, x)))
    print(labels)
    assert f"mfma_q8x_kernel<{t}>" in labels and any(l.startswith("prep_act_q8x_kernel") for l in labels)
    assert not any(re.match(r"mfma_(regb|skinny|r64)", l) for l in labels)


def test_q8_exact_supported(qmm):
    assert [qmm.q8_exact_supported(t, k) for t in MORE for k in (256, 4096)] == [1] * 6
    assert [qmm.q8_exact_supported(t, 128) for t in MORE] == [0, 0, 0]


# ----------------------------------------------------------------------------- 6. groups

def test_group_is_each_matrix_own_exact_mul_mat(qmm):
    """[Q3_K, Q4_0, Q2_K, Q4_K] on one x: every member is bit for bit its own mul_mat in q8 mode.  A prep is shared by the entries that
    follow each other with one key (prefill_group_plan): Q2_K and Q4_K run on one prep_act_q8x_kernel; Q3_K, in front of the Q4_0 member
    whose default-mode operand takes the workspace in between, has its own."""
    k, n = 2048, 130
    spec = ((Q3_K, 200), (Q4_0, 70), (Q2_K, 130), (Q4_K, 96))
    xd = dev(uniform(3, n, k))
    wd = [dev(synth.synth_weights(t, m, k, seed=30 + i, sigma=0.3)) for i, (t, m) in enumerate(spec)]
    outs = [torch.empty((n, m), dtype=torch.float32, device="cuda") for _, m in spec]
    group = lambda: qmm.mul_mat_group([(t, w) for (t, _), w in zip(spec, wd)], k, xd, outs)
    exact(qmm, group)
    for (t, m), w, o in zip(spec, wd, outs):
        assert torch.equal(o, exact(qmm, lambda: qmm.mul_mat(t, w, k, xd))), (TYPE_NAMES[t], m)
    labels = exact(qmm, lambda: qmm.trace(group))
    print(labels)
    kernels = [l for l in labels if l.startswith(("prep_", "mfma_"))]
    at = {t: kernels.index(f"mfma_q8x_kernel<{t}>") for t in (Q3_K, Q2_K, Q4_K)}
    assert kernels[at[Q3_K] - 1] == "prep_act_q8x_kernel" and kernels[at[Q2_K] - 1] == "prep_act_q8x_kernel"
    assert at[Q4_K] == at[Q2_K] + 1                              # no prep between the two: they share the one in front of Q2_K
    assert kernels.count("prep_act_q8x_kernel") == 2


# ----------------------------------------------------------------------------- 7. through the plugin (GGML_MI355X_PREC=q8 in a child's environment)

ROOT = Path(__file__).resolve().parents[1]
REF = ROOT / "oracle" / "_ref"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"


def child(exe, *args, timeout, prec="q8"):
    if not (REF / exe).exists() or not PLUGIN.exists():
        pytest.skip(f"oracle/_ref/{exe} or the plugin module is not built (needs the reference tree at build time)")
    env = {k: v for k, v in os.environ.items() if k != "GGML_MI355X_PREC"}
    env["GGML_BACKEND_PATH"] = str(PLUGIN)
    if prec:
        env["GGML_MI355X_PREC"] = prec
    p = subprocess.run([str(REF / exe), *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(REF))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr), p.stdout


def test_reference_harness_passes_in_the_exact_mode():
    rc, out, _ = child("test-backend-ops", "test", "-o", "MUL_MAT", "-p", "type_a=(q2_K|q3_K|iq4_xs),type_b=f32", timeout=600)
    assert "MI355X0" in out, out[-2000:]
    fail = [l for l in out.splitlines() if "FAIL" in l or "ERR =" in l]
    assert not fail, "\n".join(fail[:20])
    unsupported = [l for l in out.splitlines() if "not supported" in l]
    assert not unsupported, "\n".join(unsupported[:20])
    assert rc == 0, out[-3000:]
    assert len(re.findall(r"\): OK", out)) > 0


def write_tiny_llama(path, n_layer=2, n_embd=1024, n_ff=2816, n_head=8, n_head_kv=2, n_vocab=4096):
    """the tiny llama of tests/cpp/llama_e2e.cpp with the layer matmul tensors a stock Q3_K / Q2_K / IQ4_XS file keeps in those types
    (random valid blocks of sigma 0.02, ggml_hexagon_amd.synth); token_embd Q4_K and output Q6_K, norms F32"""
    rng = np.random.default_rng(0)
    kv_dim = n_embd // n_head * n_head_kv
    seed = iter(range(100, 200))

    def mat(name, t, k, m):
        return (name, t, (k, m), synth.synth_weights(t, m, k, seed=next(seed), sigma=0.02))

    def norm(name):
        return (name, gguf_synth.GGML_F32, (n_embd,), (1 + 0.05 * rng.standard_normal(n_embd)).astype(np.float32))

    tensors = [mat("token_embd.weight", Q4_K, n_embd, n_vocab), norm("output_norm.weight"), mat("output.weight", Q6_K, n_embd, n_vocab)]
    for i in range(n_layer):
        b = f"blk.{i}."
        tensors += [norm(b + "attn_norm.weight"), mat(b + "attn_q.weight", Q3_K, n_embd, n_embd), mat(b + "attn_k.weight", Q3_K, n_embd, kv_dim),
                    mat(b + "attn_v.weight", IQ4_XS, n_embd, kv_dim), mat(b + "attn_output.weight", IQ4_XS, n_embd, n_embd), norm(b + "ffn_norm.weight"),
                    mat(b + "ffn_gate.weight", Q2_K, n_embd, n_ff), mat(b + "ffn_down.weight", Q3_K, n_ff, n_embd), mat(b + "ffn_up.weight", Q2_K, n_embd, n_ff)]
    kvs = [("general.architecture", "llama"), ("general.name", "tiny-q2k-q3k-iq4xs"), ("general.file_type", 12),       # LLAMA_FTYPE_MOSTLY_Q3_K_M
           ("llama.context_length", 8192), ("llama.embedding_length", n_embd), ("llama.block_count", n_layer),
           ("llama.feed_forward_length", n_ff), ("llama.attention.head_count", n_head), ("llama.attention.head_count_kv", n_head_kv),
           ("llama.attention.layer_norm_rms_epsilon", 1e-5), ("llama.rope.dimension_count", n_embd // n_head),
           ("llama.rope.freq_base", 10000.0), ("llama.vocab_size", n_vocab), ("tokenizer.ggml.model", "no_vocab")]
    gguf_synth.write_gguf(path, kvs, tensors)
    return str(path)


def test_llama_prompt_in_the_exact_mode(tmp_path):
    """one prompt batch of 64 tokens through libllama and the plugin, logits against the CPU backend: the reference's own bar for a
    backend, NMSE <= 5e-4 (test-backend-ops), in q8 mode; the default mode's figure beside it"""
    if not (REF / "llama-e2e").exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/llama-e2e or the plugin module is not built (needs the reference tree at build time)")
    path = write_tiny_llama(tmp_path / "tiny-q2k-q3k-iq4xs.gguf")
    nmse = {}
    for prec in ("q8", None):
        rc, out, stdout = child("llama-e2e", "compare", "--gguf", path, "-p", "64", "-n", "0", "-t", "8", timeout=600, prec=prec)
        assert rc == 0, out[-3000:]
        r = json.loads([l for l in stdout.splitlines() if l.startswith("{")][-1])
        assert "MI355X0" in r["devices"]
        nmse[prec or "default"] = r["worst_nmse"]
    print("worst NMSE of the prompt's logits: q8 mode", nmse["q8"], "default mode", nmse["default"])
    assert nmse["q8"] <= 5e-4, nmse
