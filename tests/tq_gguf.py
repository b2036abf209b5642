"""Two tiny llama-arch models in the stock layouts of the ternary file types, read off the reference's src/llama-quant.cpp, written with
tests/gguf_synth.py's writer (it takes 3-D tensors as they are) and quantized by the reference's own ggml_quantize_chunk
(tests/tq_refs.py); norms and the expert router F32.  A stock TQ file is the opposite of an IQ file: every matmul tensor is TQ.

"tq2_0": the dense tiny llama of tests/iq1_gguf.py as LLAMA_FTYPE_MOSTLY_TQ2_0 (general.file_type 37):
  token_embd           Q4_K       :184-186
  output               Q6_K       :166-168
  every other matmul tensor  TQ2_0   :492-493 (the file type's default; none of the per-tensor rules names the ternary file types)
"tq1_0_moe": the 8-expert model (2 used, 2 layers) of tests/iq1_gguf.py as LLAMA_FTYPE_MOSTLY_TQ1_0 (general.file_type 36):
  attn_k, attn_v       Q8_0       :244-255 (n_expert == 8)
  token_embd           Q4_K, output Q6_K, as above
  attn_q, attn_output, ffn_gate_exps, ffn_down_exps, ffn_up_exps   TQ1_0
  ffn_gate_inp         F32        (the router is never quantized)
The TQ quantizers are a rounding per weight, so every row is quantized (no repetition)."""
import numpy as np

import gguf_synth
from iq1_gguf import DIMS as IQ1_DIMS

F32, Q8_0, Q4_K, Q6_K, TQ1_0, TQ2_0 = 0, 8, 12, 14, 34, 35
FTYPE = {"tq1_0_moe": 36, "tq2_0": 37}            # LLAMA_FTYPE_MOSTLY_TQ1_0, LLAMA_FTYPE_MOSTLY_TQ2_0
DIMS = {"tq1_0_moe": IQ1_DIMS["iq1_m_moe"], "tq2_0": IQ1_DIMS["iq1_s"]}


def layout(kind):
    """(name, ggml type, K, M, experts or 0) of every matmul tensor and of token_embd; token_embd, which llama.cpp keeps with the host,
    first in the file (the span a mapped host buffer reports is then the bytes the host holds)"""
    c = DIMS[kind]
    n_embd, n_ff, ne = c["n_embd"], c["n_ff"], c["n_expert"]
    kv_dim = n_embd // c["n_head"] * c["n_head_kv"]
    tq = TQ1_0 if kind == "tq1_0_moe" else TQ2_0
    kv = Q8_0 if ne else tq
    t = [("token_embd.weight", Q4_K, n_embd, c["n_vocab"], 0), ("output.weight", Q6_K, n_embd, c["n_vocab"], 0)]
    for i in range(c["n_layer"]):
        b = f"blk.{i}."
        t += [(b + "attn_q.weight", tq, n_embd, n_embd, 0), (b + "attn_k.weight", kv, n_embd, kv_dim, 0),
              (b + "attn_v.weight", kv, n_embd, kv_dim, 0), (b + "attn_output.weight", tq, n_embd, n_embd, 0)]
        if ne:
            t += [(b + "ffn_gate_exps.weight", tq, n_embd, n_ff, ne), (b + "ffn_down_exps.weight", tq, n_ff, n_embd, ne),
                  (b + "ffn_up_exps.weight", tq, n_embd, n_ff, ne)]
        else:
            t += [(b + "ffn_gate.weight", tq, n_embd, n_ff, 0), (b + "ffn_down.weight", tq, n_ff, n_embd, 0), (b + "ffn_up.weight", tq, n_embd, n_ff, 0)]
    return t


def write_tiny_llama(kind, path, ref, seed=0):
    """kind: "tq1_0_moe" or "tq2_0"; ref: tq_refs.TqRef.  Returns (path, bytes of the matmul tensors and token_embd by name)"""
    c = DIMS[kind]
    n_embd, n_layer = c["n_embd"], c["n_layer"]
    rng = np.random.default_rng(seed)
    tensors, sizes = [], {}
    for name, typ, k, m, ne in layout(kind):
        planes = [ref.quantize(typ, rng.standard_normal((m, k), np.float32) * np.float32(0.02)) for _ in range(max(ne, 1))]
        data = np.stack(planes) if ne else planes[0]
        tensors.append((name, typ, (k, m, ne) if ne else (k, m), data))
        sizes[name] = data.nbytes
    norms = ["output_norm.weight"] + [f"blk.{i}.{n}_norm.weight" for i in range(n_layer) for n in ("attn", "ffn")]
    for name in norms:
        tensors.append((name, F32, (n_embd,), (1 + 0.05 * rng.standard_normal(n_embd)).astype(np.float32)))
    if c["n_expert"]:
        for i in range(n_layer):
            tensors.append((f"blk.{i}.ffn_gate_inp.weight", F32, (n_embd, c["n_expert"]), rng.standard_normal((c["n_expert"], n_embd), np.float32) * np.float32(0.05)))
    kvs = [("general.architecture", "llama"), ("general.name", f"tiny-{kind}"), ("general.file_type", FTYPE[kind]),
           ("llama.context_length", 8192), ("llama.embedding_length", n_embd), ("llama.block_count", n_layer),
           ("llama.feed_forward_length", c["n_ff"]), ("llama.attention.head_count", c["n_head"]), ("llama.attention.head_count_kv", c["n_head_kv"]),
           ("llama.attention.layer_norm_rms_epsilon", 1e-5), ("llama.rope.dimension_count", n_embd // c["n_head"]),
           ("llama.rope.freq_base", 10000.0), ("llama.vocab_size", c["n_vocab"]), ("tokenizer.ggml.model", "no_vocab")]
    if c["n_expert"]:
        kvs += [("llama.expert_count", c["n_expert"]), ("llama.expert_used_count", c["n_used"])]
    gguf_synth.write_gguf(path, kvs, tensors)
    return path, sizes
