"""The tiny llama model of tests/cpp/llama_e2e.cpp as a stock IQ3_XXS file lays its tensors out (src/llama-quant.cpp:179-353), written with
tests/gguf_synth.py's writer and quantized by the reference's own ggml_quantize_chunk (tests/iq3_refs.py): attn_q / attn_k / ffn_gate /
ffn_up IQ3_XXS, attn_output / ffn_down IQ3_S, attn_v Q4_K, output Q6_K, token_embd IQ3_S, norms F32; general.file_type 23."""
import numpy as np

import gguf_synth

F32, Q4_K, Q6_K, IQ3_XXS, IQ3_S = 0, 12, 14, 18, 21
FTYPE_IQ3_XXS = 23                                # LLAMA_FTYPE_MOSTLY_IQ3_XXS


def layout(n_layer=2, n_embd=1024, n_ff=2816, n_head=8, n_head_kv=2, n_vocab=4096):
    """(name, ggml type, K, M) of every matmul tensor and of token_embd, in file order"""
    kv_dim = n_embd // n_head * n_head_kv
    t = [("token_embd.weight", IQ3_S, n_embd, n_vocab), ("output.weight", Q6_K, n_embd, n_vocab)]
    for i in range(n_layer):
        b = f"blk.{i}."
        t += [(b + "attn_q.weight", IQ3_XXS, n_embd, n_embd), (b + "attn_k.weight", IQ3_XXS, n_embd, kv_dim), (b + "attn_v.weight", Q4_K, n_embd, kv_dim),
              (b + "attn_output.weight", IQ3_S, n_embd, n_embd), (b + "ffn_gate.weight", IQ3_XXS, n_embd, n_ff),
              (b + "ffn_down.weight", IQ3_S, n_ff, n_embd), (b + "ffn_up.weight", IQ3_XXS, n_embd, n_ff)]
    return t


def write_tiny_llama_iq3(path, ref, n_layer=2, n_embd=1024, n_ff=2816, n_head=8, n_head_kv=2, n_vocab=4096, seed=0, repeat=4):
    """ref: iq3_refs.Iq3Ref.  Returns (path, bytes of the matmul tensors by name).  The i-quant quantizer searches the grid per group of
    weights and is slow, so a tensor is M / repeat quantized rows laid out `repeat` times: the same blocks a whole quantization would
    hold, a quarter of the time."""
    rng = np.random.default_rng(seed)
    tensors, sizes = [], {}
    for name, typ, k, m in layout(n_layer, n_embd, n_ff, n_head, n_head_kv, n_vocab):
        assert m % repeat == 0
        data = np.tile(ref.quantize(typ, rng.standard_normal((m // repeat, k), np.float32) * np.float32(0.02)), (repeat, 1))
        tensors.append((name, typ, (k, m), data))
        sizes[name] = data.nbytes
    norms = ["output_norm.weight"] + [f"blk.{i}.{n}_norm.weight" for i in range(n_layer) for n in ("attn", "ffn")]
    for name in norms:
        tensors.append((name, F32, (n_embd,), (1 + 0.05 * rng.standard_normal(n_embd)).astype(np.float32)))
    kvs = [("general.architecture", "llama"), ("general.name", "tiny-iq3_xxs"), ("general.file_type", FTYPE_IQ3_XXS),
           ("llama.context_length", 8192), ("llama.embedding_length", n_embd), ("llama.block_count", n_layer),
           ("llama.feed_forward_length", n_ff), ("llama.attention.head_count", n_head), ("llama.attention.head_count_kv", n_head_kv),
           ("llama.attention.layer_norm_rms_epsilon", 1e-5), ("llama.rope.dimension_count", n_embd // n_head),
           ("llama.rope.freq_base", 10000.0), ("llama.vocab_size", n_vocab), ("tokenizer.ggml.model", "no_vocab")]
    gguf_synth.write_gguf(path, kvs, tensors)
    return path, sizes
