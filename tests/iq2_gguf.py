"""The tiny llama model of tests/cpp/llama_e2e.cpp in two stock layouts that hold IQ2_XS / IQ2_S tensors, read off the reference's
src/llama-quant.cpp for this model (n_gqa = 8 / 2 = 4, no experts, 2 layers), written with tests/gguf_synth.py's writer and quantized by
the reference's own ggml_quantize_chunk (tests/iq2_refs.py); norms F32.

LLAMA_FTYPE_MOSTLY_IQ3_XXS (general.file_type 23), as a file made with an importance matrix has it:
  attn_q, attn_k       IQ2_S      :259-268
  attn_v               Q4_K       :219-221 (n_gqa >= 4)
  attn_output          IQ3_S      :323-325
  ffn_gate, ffn_up     IQ3_XXS    the file type's default (:341-356 change IQ3_XS files only)
  ffn_down             IQ3_XXS    the default: :276-278 replace it (by Q3_K here, layer >= n_layer / 8) only in a file made without an
                                  importance matrix
  output               Q5_K       :161-165
  token_embd           IQ3_S      :181-183
LLAMA_FTYPE_MOSTLY_IQ2_XS (general.file_type 20; default type IQ2_XS):
  attn_v               Q4_K       :190-191 (n_gqa >= 4)
  ffn_down             IQ2_XS     :198-201 raise only the layers below n_ffn_down / 8 = 0
  attn_q, attn_k, attn_output, ffn_gate, ffn_up   IQ2_XS   (:204-211 change attn_output for the IQ1 and IQ2_S / IQ2_M files only)
  output               Q5_K       :161-165
  token_embd           Q2_K       :174-177"""
import numpy as np

import gguf_synth

F32, Q2_K, Q4_K, Q5_K, IQ2_XS, IQ3_XXS, IQ3_S, IQ2_S = 0, 10, 12, 13, 17, 18, 21, 22
FTYPE = {"iq3_xxs": 23, "iq2_xs": 20}             # LLAMA_FTYPE_MOSTLY_IQ3_XXS, LLAMA_FTYPE_MOSTLY_IQ2_XS
TYPES = {"iq3_xxs": dict(token_embd=IQ3_S, output=Q5_K, attn_q=IQ2_S, attn_k=IQ2_S, attn_v=Q4_K, attn_output=IQ3_S,
                         ffn_gate=IQ3_XXS, ffn_down=IQ3_XXS, ffn_up=IQ3_XXS),
         "iq2_xs": dict(token_embd=Q2_K, output=Q5_K, attn_q=IQ2_XS, attn_k=IQ2_XS, attn_v=Q4_K, attn_output=IQ2_XS,
                        ffn_gate=IQ2_XS, ffn_down=IQ2_XS, ffn_up=IQ2_XS)}


def layout(kind, n_layer=2, n_embd=1024, n_ff=2816, n_head=8, n_head_kv=2, n_vocab=4096):
    """(name, ggml type, K, M) of every matmul tensor and of token_embd, in file order"""
    ty = TYPES[kind]
    kv_dim = n_embd // n_head * n_head_kv
    t = [("token_embd.weight", ty["token_embd"], n_embd, n_vocab), ("output.weight", ty["output"], n_embd, n_vocab)]
    for i in range(n_layer):
        b = f"blk.{i}."
        t += [(b + "attn_q.weight", ty["attn_q"], n_embd, n_embd), (b + "attn_k.weight", ty["attn_k"], n_embd, kv_dim),
              (b + "attn_v.weight", ty["attn_v"], n_embd, kv_dim), (b + "attn_output.weight", ty["attn_output"], n_embd, n_embd),
              (b + "ffn_gate.weight", ty["ffn_gate"], n_embd, n_ff), (b + "ffn_down.weight", ty["ffn_down"], n_ff, n_embd),
              (b + "ffn_up.weight", ty["ffn_up"], n_embd, n_ff)]
    return t


def write_tiny_llama(kind, path, ref, n_layer=2, n_embd=1024, n_ff=2816, n_head=8, n_head_kv=2, n_vocab=4096, seed=0, repeat=16):
    """kind: "iq3_xxs" or "iq2_xs"; ref: iq2_refs.Iq2Ref (its quantize passes the importance matrix IQ2_XS needs, all ones).  Returns
    (path, bytes of the matmul tensors by name).  The i-quant quantizers search the grid per group of weights and are slow, so a tensor
    is M / repeat quantized rows laid out `repeat` times: the same blocks a whole quantization would hold, a sixteenth of the time."""
    rng = np.random.default_rng(seed)
    tensors, sizes = [], {}
    for name, typ, k, m in layout(kind, n_layer, n_embd, n_ff, n_head, n_head_kv, n_vocab):
        assert m % repeat == 0
        data = np.tile(ref.quantize(typ, rng.standard_normal((m // repeat, k), np.float32) * np.float32(0.02)), (repeat, 1))
        tensors.append((name, typ, (k, m), data))
        sizes[name] = data.nbytes
    norms = ["output_norm.weight"] + [f"blk.{i}.{n}_norm.weight" for i in range(n_layer) for n in ("attn", "ffn")]
    for name in norms:
        tensors.append((name, F32, (n_embd,), (1 + 0.05 * rng.standard_normal(n_embd)).astype(np.float32)))
    kvs = [("general.architecture", "llama"), ("general.name", f"tiny-{kind}"), ("general.file_type", FTYPE[kind]),
           ("llama.context_length", 8192), ("llama.embedding_length", n_embd), ("llama.block_count", n_layer),
           ("llama.feed_forward_length", n_ff), ("llama.attention.head_count", n_head), ("llama.attention.head_count_kv", n_head_kv),
           ("llama.attention.layer_norm_rms_epsilon", 1e-5), ("llama.rope.dimension_count", n_embd // n_head),
           ("llama.rope.freq_base", 10000.0), ("llama.vocab_size", n_vocab), ("tokenizer.ggml.model", "no_vocab")]
    gguf_synth.write_gguf(path, kvs, tensors)
    return path, sizes
