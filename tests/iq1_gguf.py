"""Two tiny llama-arch models in the stock layouts that hold IQ1_S / IQ1_M tensors, read off the reference's src/llama-quant.cpp,
written with tests/gguf_synth.py's writer (it takes 3-D tensors as they are) and quantized by the reference's own ggml_quantize_chunk
(tests/iq1_refs.py, importance matrix of ones); norms and the expert router F32.

"iq1_m_moe": an 8-expert model (2 used, 2 layers) as LLAMA_FTYPE_MOSTLY_IQ1_M (general.file_type 31) lays it out:
  attn_v               Q4_K       :190-191 (n_expert >= 4)
  attn_k               Q4_K       :195-196 (n_expert == 8)
  ffn_down_exps        IQ1_M      :198-203 raise only the layers below n_ffn_down / 8 = 2 / 8 = 0
  attn_output          Q5_K       :204-206 (n_expert == 8)
  attn_q, ffn_gate_exps, ffn_up_exps   IQ1_M   the file type's default
  output               Q5_K       :161-165
  token_embd           Q2_K       :174-177
  ffn_gate_inp         F32        (the router is never quantized)
"iq1_s": the dense tiny llama of tests/iq2_gguf.py (n_gqa = 4, no experts) as LLAMA_FTYPE_MOSTLY_IQ1_S (general.file_type 24):
  attn_v               Q4_K       :190-191 (n_gqa >= 4)
  attn_output          IQ2_XXS    :207-208 - a type the device does not run: this one tensor per layer stays with the CPU backend
  ffn_down             IQ1_S      :198-203, as above
  attn_q, attn_k, ffn_gate, ffn_up   IQ1_S
  output               Q5_K       :161-165
  token_embd           Q2_K       :174-177"""
import numpy as np

import gguf_synth

F32, Q2_K, Q4_K, Q5_K, IQ2_XXS, IQ1_S, IQ1_M = 0, 10, 12, 13, 16, 19, 29
FTYPE = {"iq1_m_moe": 31, "iq1_s": 24}            # LLAMA_FTYPE_MOSTLY_IQ1_M, LLAMA_FTYPE_MOSTLY_IQ1_S
DIMS = {"iq1_m_moe": dict(n_layer=2, n_embd=512, n_ff=512, n_head=8, n_head_kv=2, n_vocab=2048, n_expert=8, n_used=2),
        "iq1_s": dict(n_layer=2, n_embd=1024, n_ff=2816, n_head=8, n_head_kv=2, n_vocab=4096, n_expert=0, n_used=0)}


def layout(kind):
    """(name, ggml type, K, M, experts or 0) of every matmul tensor and of token_embd, in file order (the order of a model's tensors in a
    GGUF is free; the loader finds them by name)"""
    c = DIMS[kind]
    n_embd, n_ff, ne = c["n_embd"], c["n_ff"], c["n_expert"]
    kv_dim = n_embd // c["n_head"] * c["n_head_kv"]
    iq = IQ1_M if kind == "iq1_m_moe" else IQ1_S
    t = [("token_embd.weight", Q2_K, n_embd, c["n_vocab"], 0), ("output.weight", Q5_K, n_embd, c["n_vocab"], 0)]
    for i in range(c["n_layer"]):
        b = f"blk.{i}."
        t += [(b + "attn_q.weight", iq, n_embd, n_embd, 0), (b + "attn_k.weight", Q4_K if ne else iq, n_embd, kv_dim, 0),
              (b + "attn_v.weight", Q4_K, n_embd, kv_dim, 0), (b + "attn_output.weight", Q5_K if ne else IQ2_XXS, n_embd, n_embd, 0)]
        if ne:
            t += [(b + "ffn_gate_exps.weight", iq, n_embd, n_ff, ne), (b + "ffn_down_exps.weight", iq, n_ff, n_embd, ne),
                  (b + "ffn_up_exps.weight", iq, n_embd, n_ff, ne)]
        else:
            t += [(b + "ffn_gate.weight", iq, n_embd, n_ff, 0), (b + "ffn_down.weight", iq, n_ff, n_embd, 0), (b + "ffn_up.weight", iq, n_embd, n_ff, 0)]
    # what stays with the host goes first in the file: llama.cpp reports a mapped host buffer as the span from the first to the last
    # host tensor of the file, so only with these side by side is that figure the bytes the host holds (tests/test_gpu_iq1_e2e.py)
    return sorted(t, key=lambda e: not (e[0] == "token_embd.weight" or e[1] == IQ2_XXS))


def write_tiny_llama(kind, path, ref, seed=0, repeat=32):
    """kind: "iq1_m_moe" or "iq1_s"; ref: iq1_refs.Iq1Ref.  Returns (path, bytes of the matmul tensors by name).  The IQ1 quantizers
    search the grid per group of weights and are the slowest of all, so a tensor (of the MoE model: each expert) is M / repeat quantized
    rows laid out `repeat` times: the same blocks a whole quantization would hold, in a fraction of the time.  Experts get rows of
    their own, so routing to the wrong expert shows."""
    c = DIMS[kind]
    n_embd, n_layer = c["n_embd"], c["n_layer"]
    rng = np.random.default_rng(seed)
    tensors, sizes = [], {}
    for name, typ, k, m, ne in layout(kind):
        assert m % repeat == 0
        planes = [np.tile(ref.quantize(typ, rng.standard_normal((m // repeat, k), np.float32) * np.float32(0.02)), (repeat, 1)) for _ in range(max(ne, 1))]
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
