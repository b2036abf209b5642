"""QMM_PREC_Q8_EXACT: the opt-in prefill mode that forms the integers of ggml_vec_dot_q{4,5,6}_K_q8_K on the int8 MFMA and converts them
to f32 once per 256-element superblock (include/ggml_mi355x_qmm.h, csrc/qmm_mfma_q8x.hiph).

Bar: the project's bar for "only the f32 summation order differs from the CPU backend", max |err| / rms(want) <= 2e-5 (test_gpu_parity.py);
`want` is always the CPU oracle on ACT_REF activations.  The same calls in the default mode (f16 operands) sit near 2e-3, and before the
mode existed set_precision(2) was QMM_EINVAL.  Calls the mode does not cover (other weight types, MUL_MAT_ID) must be the default mode's
launches and bits."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ggml_hexagon_amd.synth as synth  # noqa: E402
from oracle.pyoracle import ACT_REF, Q4_0, Q4_K, Q5_K, Q6_K, Q8_0, TYPE_NAMES  # noqa: E402

EXACT = (Q4_K, Q5_K, Q6_K)
IDS = [TYPE_NAMES[t] for t in EXACT]
BAR = 2e-5
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


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


def exact(qmm, fn):
    """fn() in the exact mode; the context is back in the default mode afterwards, whatever happens"""
    qmm.set_precision(PREC_Q8_EXACT)
    try:
        return fn()
    finally:
        qmm.set_precision(PREC_F16_Q8)


def uniform(seed, n, k):
    return np.random.default_rng(seed).uniform(-1, 1, (n, k)).astype(np.float32)


# ----------------------------------------------------------------------------- 1. parity grid

@pytest.mark.parametrize("t", EXACT, ids=IDS)
@pytest.mark.parametrize("n", [9, 32, 33, 64, 129, 512])
def test_parity_grid(qmm, oracle, t, n):
    k, m = 2048, 200
    w = synth.synth_weights(t, m, k, seed=20 + t, sigma=0.3)
    x = uniform(n, n, k)
    got = exact(qmm, lambda: qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy())
    err = rel_rms(got, oracle.mul_mat(t, w, k, x, ACT_REF))
    print(TYPE_NAMES[t], n, err)
    assert err <= BAR, err


# ----------------------------------------------------------------------------- 2. ragged and edge shapes

@pytest.mark.parametrize("t", EXACT, ids=IDS)
@pytest.mark.parametrize("m,k,n", [(16, 256, 9), (512, 256, 32), (77, 1024, 130), (130, 512, 257), (48, 14336, 96)])
def test_ragged_and_edge_shapes(qmm, oracle, t, m, k, n):
    w = synth.synth_weights(t, m, k, seed=m, sigma=0.2)
    x = uniform(n, n, k)
    got = exact(qmm, lambda: qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy())
    err = rel_rms(got, oracle.mul_mat(t, w, k, x, ACT_REF))
    print(TYPE_NAMES[t], (m, k, n), err)
    assert err <= BAR, err


@pytest.mark.parametrize("t", EXACT, ids=IDS)
def test_strided_destination_and_padded_weight_rows(qmm, oracle, t):
    m, k, n = 77, 1024, 130
    w = synth.synth_weights(t, m, k, seed=7, sigma=0.2)
    x = uniform(5, n, k)
    want = oracle.mul_mat(t, w, k, x, ACT_REF)
    big = torch.full((n, m + 8), 3.0, device="cuda")
    exact(qmm, lambda: qmm.mul_mat(t, dev(w), k, dev(x), out=big[:, :m]))
    assert (big[:, m:] == 3.0).all()
    assert rel_rms(big[:, :m].cpu().numpy(), want) <= BAR
    # weight rows further apart than the packed row (w_row_bytes = w.stride(0)); the spare bytes hold what no block may hold
    wide = torch.full((m, w.shape[1] + 6), 0xFF, dtype=torch.uint8, device="cuda")
    wide[:, :w.shape[1]] = dev(w)
    got = exact(qmm, lambda: qmm.mul_mat(t, wide[:, :w.shape[1]], k, dev(x)).cpu().numpy())
    assert rel_rms(got, want) <= BAR


# ----------------------------------------------------------------------------- 3. integer range edges

def edge_x(k, n=40):
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    x[:8] = 1.0
    x[8:16] = -1.0
    x[16:24] = np.abs(x[16:24])
    return x                                                     # whole rows of q8 at +127 / -127


def f16_bytes(v):
    return np.array([v], np.float16).view(np.uint8)


@pytest.mark.parametrize("t", (Q4_K, Q5_K), ids=["q4_K", "q5_K"])
def test_range_edge_q4k_q5k_largest_scale_min_and_weight(qmm, oracle, t):
    """every byte 0xFF: sc = m = 63 in every sub-block, q = 15 / 31: the top of the hi plane (7 / 15) and of the mins plane"""
    m, k = 40, 2048
    blk = np.full(synth.TYPE_SIZE[t], 0xFF, np.uint8)
    blk[0:2] = f16_bytes(2.0 ** -6)
    blk[2:4] = f16_bytes(2.0 ** -8)
    w = np.tile(blk, (m, k // 256))
    x = edge_x(k)
    want = oracle.mul_mat(t, w, k, x, ACT_REF)
    got = exact(qmm, lambda: qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy())
    print(TYPE_NAMES[t], "rms", float(np.sqrt(np.mean(want.astype(np.float64) ** 2))), rel_rms(got, want))
    assert rel_rms(got, want) <= BAR


@pytest.mark.parametrize("scale", [0x80, 0x7F], ids=["sc-128", "sc+127"])
def test_range_edge_q6k_most_negative_weight(qmm, oracle, scale):
    """ql = qh = 0: q = -32; scales 0x80: sc = -128, sc * q = +4096 = 128 * 32, the top of the hi plane; 0x7F: -4064, its bottom side"""
    m, k = 40, 2048
    blk = np.zeros(210, np.uint8)
    blk[192:208] = scale
    blk[208:210] = f16_bytes(2.0 ** -8)
    w = np.tile(blk, (m, k // 256))
    x = edge_x(k)
    want = oracle.mul_mat(Q6_K, w, k, x, ACT_REF)
    got = exact(qmm, lambda: qmm.mul_mat(Q6_K, dev(w), k, dev(x)).cpu().numpy())
    print("q6_K", hex(scale), "rms", float(np.sqrt(np.mean(want.astype(np.float64) ** 2))), rel_rms(got, want))
    assert rel_rms(got, want) <= BAR


# ----------------------------------------------------------------------------- 4. beyond the f16 range

def test_block_beyond_the_f16_range_is_exact_and_raises_nothing(qmm, oracle):
    """the Q4_K block of test_f16_prefill_overflow_is_a_loud_error_and_bf16_handles_it (d = 65504): the default mode reports non-finite
    values at the next synchronize; integers have no such range"""
    k, m, n = 512, 64, 40
    w = synth.synth_weights(Q4_K, m, k, seed=3, sigma=0.05).reshape(m, -1, synth.TYPE_SIZE[Q4_K])
    w[5, 1, 0:2] = np.array([0x7BFF], np.uint16).view(np.uint8)
    w = w.reshape(m, -1)
    x = uniform(9, n, k)
    want = oracle.mul_mat(Q4_K, w, k, x, ACT_REF)
    assert np.isfinite(want).all()
    qmm.synchronize()

    def run():
        got = qmm.mul_mat(Q4_K, dev(w), k, dev(x)).cpu().numpy()
        qmm.synchronize()                                        # raises on a reported overflow
        return got
    assert rel_rms(exact(qmm, run), want) <= BAR


# ----------------------------------------------------------------------------- 5. determinism and mode isolation

@pytest.mark.parametrize("t", EXACT, ids=IDS)
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


# ----------------------------------------------------------------------------- 6. the plan is visible; what the mode does not cover falls back

def test_trace_names_the_exact_kernel(qmm):
    k, m, n = 1024, 200, 64
    w, x = dev(synth.synth_weights(Q4_K, m, k, seed=1, sigma=0.3)), dev(uniform(2, n, k))
    labels = exact(qmm, lambda: qmm.trace(lambda: qmm.mul_mat(Q4_K, w, k, x)))
    print(labels)
    assert any(l.startswith("mfma_q8x_kernel<") for l in labels) and any(l.startswith("prep_act_q8x_kernel") for l in labels)
    assert not any(re.match(r"mfma_(regb|skinny|r64)", l) for l in labels)


def test_other_weight_types_fall_back_to_the_default_mode(qmm):
    k, m, n = 1024, 200, 64
    x = dev(uniform(2, n, k))
    for t in (Q8_0, Q4_0):
        w = dev(synth.synth_weights(t, m, k, seed=1, sigma=0.3))
        want_labels = qmm.trace(lambda: qmm.mul_mat(t, w, k, x))
        want = qmm.mul_mat(t, w, k, x)
        labels = exact(qmm, lambda: qmm.trace(lambda: qmm.mul_mat(t, w, k, x)))
        assert labels == want_labels and not any("q8x" in l for l in labels)
        assert torch.equal(exact(qmm, lambda: qmm.mul_mat(t, w, k, x)), want)


def test_mul_mat_id_falls_back_to_the_default_mode(qmm):
    k, m, n_expert, n_used, n_tokens = 512, 64, 4, 2, 32
    w = dev(np.stack([synth.synth_weights(Q4_K, m, k, seed=e, sigma=0.2) for e in range(n_expert)]))
    rng = np.random.default_rng(0)
    ids = dev(np.stack([rng.permutation(n_expert) for _ in range(n_tokens)]).astype(np.int32)[:, :n_used])
    b = dev(rng.uniform(-1, 1, (n_tokens, 1, k)).astype(np.float32))
    want_labels = qmm.trace(lambda: qmm.mul_mat_id(Q4_K, w, k, b, ids))
    want = qmm.mul_mat_id(Q4_K, w, k, b, ids)
    labels = exact(qmm, lambda: qmm.trace(lambda: qmm.mul_mat_id(Q4_K, w, k, b, ids)))
    assert labels == want_labels and not any("q8x" in l for l in labels)
    assert torch.equal(exact(qmm, lambda: qmm.mul_mat_id(Q4_K, w, k, b, ids)), want)


def test_q8_exact_supported(qmm):
    assert [qmm.q8_exact_supported(t, k) for t in EXACT for k in (256, 4096)] == [1] * 6
    assert [qmm.q8_exact_supported(t, 4096) for t in (Q8_0, Q4_0)] == [0, 0]


# ----------------------------------------------------------------------------- 7. groups

def test_group_is_each_matrix_own_exact_mul_mat(qmm, oracle):
    k, n = 4096, 300
    spec = ((Q4_K, 300), (Q4_K, 70), (Q6_K, 130))
    ws = [synth.synth_weights(t, m, k, seed=30 + i, sigma=0.3) for i, (t, m) in enumerate(spec)]
    x = uniform(3, n, k)
    xd, wd = dev(x), [dev(w) for w in ws]
    outs = [torch.empty((n, m), dtype=torch.float32, device="cuda") for _, m in spec]
    exact(qmm, lambda: qmm.mul_mat_group([(t, w) for (t, _), w in zip(spec, wd)], k, xd, outs))
    for (t, m), w, wdev, o in zip(spec, ws, wd, outs):
        assert rel_rms(o.cpu().numpy(), oracle.mul_mat(t, w, k, x, ACT_REF)) <= BAR, (TYPE_NAMES[t], m)
        assert torch.equal(o, exact(qmm, lambda: qmm.mul_mat(t, wdev, k, xd)))


# ----------------------------------------------------------------------------- 8. through the plugin (GGML_MI355X_PREC=q8 in a child's environment)

ROOT = Path(__file__).resolve().parents[1]
REF = ROOT / "oracle" / "_ref"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"


def child(exe, *args, timeout):
    if not (REF / exe).exists() or not PLUGIN.exists():
        pytest.skip(f"oracle/_ref/{exe} or the plugin module is not built (needs the reference tree at build time)")
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), GGML_MI355X_PREC="q8")
    p = subprocess.run([str(REF / exe), *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(REF))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr), p.stdout


def test_reference_harness_passes_in_the_exact_mode():
    rc, out, _ = child("test-backend-ops", "test", "-o", "MUL_MAT", "-p", "type_a=(q4_K|q5_K|q6_K)", timeout=600)
    assert "MI355X0" in out, out[-2000:]
    fail = [l for l in out.splitlines() if "FAIL" in l or "ERR =" in l]
    assert not fail, "\n".join(fail[:20])
    assert rc == 0, out[-3000:]
    assert len(re.findall(r"\): OK", out)) > 0


@pytest.mark.parametrize("config", ["tiny-q4_k_m", "tiny-q4_0"])
def test_llama_logits_in_the_exact_mode(tmp_path, config):
    """a model of exact types (Q4_K / Q6_K) and one of fallback types only: the mode is safe end to end (the logits bar of test_gpu_llama_e2e.py)"""
    import json
    path = str(tmp_path / f"{config}.gguf")
    rc, out, _ = child("llama-e2e", "write", "--config", config, "--gguf", path, timeout=300)
    assert rc == 0, out[-3000:]
    rc, out, stdout = child("llama-e2e", "compare", "--gguf", path, "-p", "64", "-n", "8", "-t", "8", timeout=600)
    assert rc == 0, out[-3000:]
    r = json.loads([l for l in stdout.splitlines() if l.startswith("{")][-1])
    print(r)
    assert "MI355X0" in r["devices"]
    assert r["worst_nmse"] < 5e-3, r
