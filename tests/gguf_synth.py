"""A minimal GGUF v3 writer of our own, and the tiny llama model of tests/cpp/llama_e2e.cpp with BF16 weights.

Format (ggml/docs/gguf.md): little-endian; magic "GGUF", version u32 = 3, tensor count u64, KV count u64; each KV = key string (u64 length +
bytes), value type u32 (u32 = 4, f32 = 6, string = 8), value; each tensor info = name string, n_dims u32, ne[] u64, ggml type u32,
offset u64 relative to the data section; the data section starts at the next multiple of the alignment (32), and every tensor in it too."""
import struct

import numpy as np

ALIGN = 32
GGML_F32, GGML_BF16 = 0, 30
KV_U32, KV_F32, KV_STR = 4, 6, 8


def _s(text):
    b = text.encode()
    return struct.pack("<Q", len(b)) + b


def _kv(key, value):
    if isinstance(value, str):
        return _s(key) + struct.pack("<I", KV_STR) + _s(value)
    if isinstance(value, float):
        return _s(key) + struct.pack("<If", KV_F32, value)
    return _s(key) + struct.pack("<II", KV_U32, value)


def f32_to_bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def write_gguf(path, kvs, tensors):
    """kvs: list of (key, str | float | int); tensors: list of (name, ggml type, ne tuple (ne[0] first), numpy array of the raw data)"""
    head = b"GGUF" + struct.pack("<IQQ", 3, len(tensors), len(kvs)) + b"".join(_kv(k, v) for k, v in kvs)
    infos, off = b"", 0
    for name, typ, ne, data in tensors:
        infos += _s(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", n) for n in ne) + struct.pack("<IQ", typ, off)
        off += (data.nbytes + ALIGN - 1) // ALIGN * ALIGN
    with open(path, "wb") as f:
        f.write(head + infos)
        f.write(b"\0" * (-f.tell() % ALIGN))
        for _, _, _, data in tensors:
            f.write(np.ascontiguousarray(data).tobytes())
            f.write(b"\0" * (-data.nbytes % ALIGN))


def write_tiny_llama_bf16(path, n_layer=2, n_embd=1024, n_ff=2816, n_head=8, n_head_kv=2, n_vocab=4096, seed=0):
    """the model of llama_e2e.cpp's tiny configs (same metadata keys): matmul tensors and token_embd BF16 from N(0, 0.02), norms F32 N(1, 0.05)"""
    rng = np.random.default_rng(seed)
    kv_dim = n_embd // n_head * n_head_kv

    def mat(name, k, m):
        return (name, GGML_BF16, (k, m), f32_to_bf16((rng.standard_normal((m, k), np.float32) * np.float32(0.02))))

    def norm(name):
        return (name, GGML_F32, (n_embd,), (1 + 0.05 * rng.standard_normal(n_embd)).astype(np.float32))

    tensors = [mat("token_embd.weight", n_embd, n_vocab), norm("output_norm.weight"), mat("output.weight", n_embd, n_vocab)]
    for i in range(n_layer):
        b = f"blk.{i}."
        tensors += [norm(b + "attn_norm.weight"), mat(b + "attn_q.weight", n_embd, n_embd), mat(b + "attn_k.weight", n_embd, kv_dim),
                    mat(b + "attn_v.weight", n_embd, kv_dim), mat(b + "attn_output.weight", n_embd, n_embd), norm(b + "ffn_norm.weight"),
                    mat(b + "ffn_gate.weight", n_embd, n_ff), mat(b + "ffn_down.weight", n_ff, n_embd), mat(b + "ffn_up.weight", n_embd, n_ff)]
    kvs = [("general.architecture", "llama"), ("general.name", "tiny-bf16"), ("general.file_type", 32),          # LLAMA_FTYPE_MOSTLY_BF16
           ("llama.context_length", 8192), ("llama.embedding_length", n_embd), ("llama.block_count", n_layer),
           ("llama.feed_forward_length", n_ff), ("llama.attention.head_count", n_head), ("llama.attention.head_count_kv", n_head_kv),
           ("llama.attention.layer_norm_rms_epsilon", 1e-5), ("llama.rope.dimension_count", n_embd // n_head),
           ("llama.rope.freq_base", 10000.0), ("llama.vocab_size", n_vocab), ("tokenizer.ggml.model", "no_vocab")]
    write_gguf(path, kvs, tensors)
    return path
