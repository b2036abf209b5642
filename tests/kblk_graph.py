"""The attention block of a layer on a K cache in Q4_0, Q4_1, Q5_0 or Q5_1 (the type is an argument) and a transposed F16 V cache, built on ggml's public API through ctypes (the libraries
oracle/Makefile builds into oracle/_ref) and computed by one backend: the CPU backend or this project's plugin.  Helper of
tests/test_gpu_kblk_graph.py, which runs it in a child process per backend:

    python tests/kblk_graph.py cpu|mi355x q4_0|q4_1|q5_0|q5_1 N j0 n_kv out.npz

Two such blocks in a row (the second one's q is the first one's output; each has its own caches and its own k / v inputs), with the nodes
build_attn / build_attn_mha emit without flash attention (src/llama-graph.cpp:1306-1400, 1166-1205):
    rope(q), rope(k), cpy(k -> K cache view at row j0), cpy(v^T -> V cache view at column j0), permute(q),
    kq = mul_mat(k view, q), soft_max_ext(kq, mask, scale), kqv = mul_mat(v view, kq), permute, cont_2d
Two blocks because ggml-alloc hands the first block's buffers to the second: the plugin fuses only nodes whose readers it can prove to be
inside the graph, which it reads off such reuse, so the first block runs as a layer inside a model does and the last one as the end of a
graph does (its nodes one by one).  Shapes: H 8, H_kv 2, D 128, n_ctx 256."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
REF = ROOT / "oracle" / "_ref"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"

F32, F16, I32 = 0, 1, 26
K_TYPES = {"q4_0": (2, 18), "q4_1": (3, 20), "q5_0": (6, 22), "q5_1": (7, 24)}          # ggml type code, bytes per block of 32
H, HK, D, N_CTX, LAYERS = 8, 2, 128, 256, 2


def row_bytes(k_type):
    """bytes of a K cache row"""
    return HK * (D // 32) * K_TYPES[k_type][1]


class InitParams(C.Structure):
    _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]


def load():
    base = C.CDLL(str(REF / "libggml-base.so"), mode=C.RTLD_GLOBAL)
    cpu = C.CDLL(str(REF / "libggml-cpu.so"), mode=C.RTLD_GLOBAL)
    reg = C.CDLL(str(REF / "libggml.so"), mode=C.RTLD_GLOBAL)
    p, i64, sz, f = C.c_void_p, C.c_int64, C.c_size_t, C.c_float
    sig = {
        "ggml_init": (p, [InitParams]), "ggml_free": (None, [p]),
        "ggml_new_tensor_1d": (p, [p, C.c_int, i64]), "ggml_new_tensor_2d": (p, [p, C.c_int, i64, i64]), "ggml_new_tensor_3d": (p, [p, C.c_int, i64, i64, i64]),
        "ggml_view_1d": (p, [p, p, i64, sz]), "ggml_view_2d": (p, [p, p, i64, i64, sz, sz]), "ggml_view_3d": (p, [p, p, i64, i64, i64, sz, sz, sz]),
        "ggml_reshape_2d": (p, [p, p, i64, i64]), "ggml_reshape_3d": (p, [p, p, i64, i64, i64]),
        "ggml_permute": (p, [p, p, C.c_int, C.c_int, C.c_int, C.c_int]), "ggml_transpose": (p, [p, p]), "ggml_cpy": (p, [p, p, p]),
        "ggml_rope_ext": (p, [p, p, p, p, C.c_int, C.c_int, C.c_int, f, f, f, f, f, f]),
        "ggml_mul_mat": (p, [p, p, p]), "ggml_soft_max_ext": (p, [p, p, p, f, f]), "ggml_cont_2d": (p, [p, p, i64, i64]),
        "ggml_set_name": (p, [p, C.c_char_p]), "ggml_get_name": (C.c_char_p, [p]), "ggml_op_desc": (C.c_char_p, [p]),
        "ggml_new_graph": (p, [p]), "ggml_build_forward_expand": (None, [p, p]), "ggml_graph_n_nodes": (C.c_int, [p]), "ggml_graph_node": (p, [p, C.c_int]),
        "ggml_nbytes": (sz, [p]),
        "ggml_backend_alloc_ctx_tensors": (p, [p, p]), "ggml_backend_buffer_clear": (None, [p, C.c_uint8]), "ggml_backend_buffer_free": (None, [p]),
        "ggml_backend_get_default_buffer_type": (p, [p]), "ggml_gallocr_new": (p, [p]), "ggml_gallocr_alloc_graph": (C.c_bool, [p, p]), "ggml_gallocr_free": (None, [p]),
        "ggml_backend_tensor_set": (None, [p, p, sz, sz]), "ggml_backend_tensor_get": (None, [p, p, sz, sz]),
        "ggml_backend_graph_compute": (C.c_int, [p, p]), "ggml_backend_supports_op": (C.c_bool, [p, p]), "ggml_backend_free": (None, [p]),
        "quantize_row_q4_0_ref": (None, [p, p, i64]), "quantize_row_q4_1_ref": (None, [p, p, i64]),
        "quantize_row_q5_0_ref": (None, [p, p, i64]), "quantize_row_q5_1_ref": (None, [p, p, i64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(base, name)
        fn.restype, fn.argtypes = res, args
    cpu.ggml_backend_cpu_init.restype = p
    reg.ggml_backend_load.restype = p
    reg.ggml_backend_load.argtypes = [C.c_char_p]
    reg.ggml_backend_init_by_name.restype = p
    reg.ggml_backend_init_by_name.argtypes = [C.c_char_p, C.c_char_p]
    return base, cpu, reg


def inputs(n, j0, n_kv):
    """seeded inputs, the same for both backends: per block q (the first only), k, v [*, n] f32, and caches whose rows below j0 hold earlier tokens"""
    rng = np.random.default_rng(1000 * n + j0)
    data = {"q": rng.normal(0, 1, (n, H, D)).astype(np.float32), "pos": (j0 + np.arange(n)).astype(np.int32)}
    mask = np.full(((n + 63) // 64 * 64, n_kv), -np.inf, np.float32)
    for t in range(n):
        mask[t, :j0 + t + 1] = 0.0                                      # causal: token t sits at cache row j0 + t
    data["mask"] = mask
    for l in range(LAYERS):
        data[f"k{l}"] = rng.normal(0, 1, (n, HK, D)).astype(np.float32)
        data[f"v{l}"] = rng.normal(0, 1, (n, HK * D)).astype(np.float32)
        data[f"k_old{l}"] = rng.normal(0, 1, (j0, HK * D)).astype(np.float32)             # quantized by the reference's quantize_row_<type>_ref below
        data[f"v_old{l}"] = rng.normal(0, 1, (HK * D, j0)).astype(np.float16)
    return data


def run(backend_name, k_type, n, j0, n_kv, out_path):
    g, cpu, reg = load()
    K_CODE, ROW = K_TYPES[k_type][0], row_bytes(k_type)
    quantize_row = getattr(g, f"quantize_row_{k_type}_ref")
    if backend_name == "cpu":
        backend = cpu.ggml_backend_cpu_init()
    else:
        assert reg.ggml_backend_load(str(PLUGIN).encode()), "the plugin module does not load"
        backend = reg.ggml_backend_init_by_name(b"MI355X0", None)
    assert backend, backend_name
    data = inputs(n, j0, n_kv)
    n_pad = data["mask"].shape[0]

    # leaves: inputs and caches, in a buffer of the backend
    ctx_in = g.ggml_init(InitParams(1 << 20, None, True))
    leaves = {"q": g.ggml_new_tensor_3d(ctx_in, F32, D, H, n), "pos": g.ggml_new_tensor_1d(ctx_in, I32, n), "mask": g.ggml_new_tensor_2d(ctx_in, F32, n_kv, n_pad)}
    for l in range(LAYERS):
        leaves[f"k{l}"] = g.ggml_new_tensor_3d(ctx_in, F32, D, HK, n)
        leaves[f"v{l}"] = g.ggml_new_tensor_2d(ctx_in, F32, HK * D, n)
        leaves[f"kc{l}"] = g.ggml_new_tensor_1d(ctx_in, K_CODE, HK * D * N_CTX)
        leaves[f"vc{l}"] = g.ggml_new_tensor_1d(ctx_in, F16, HK * D * N_CTX)
    for name, t in leaves.items():
        g.ggml_set_name(t, name.encode())
    buf_in = g.ggml_backend_alloc_ctx_tensors(ctx_in, backend)
    assert buf_in
    g.ggml_backend_buffer_clear(buf_in, 0)

    def put(name, a, offset=0):
        a = np.ascontiguousarray(a)
        g.ggml_backend_tensor_set(leaves[name], a.ctypes.data_as(C.c_void_p), offset, a.nbytes)

    for name in ["q", "pos", "mask"] + [f"{x}{l}" for l in range(LAYERS) for x in "kv"]:
        put(name, data[name])
    for l in range(LAYERS):
        if j0:
            old = np.zeros((j0, ROW), np.uint8)
            for r in range(j0):
                quantize_row(data[f"k_old{l}"][r].ctypes.data_as(C.c_void_p), old[r].ctypes.data_as(C.c_void_p), HK * D)
            put(f"kc{l}", old)
            vt = np.zeros((HK * D, N_CTX), np.float16)
            vt[:, :j0] = data[f"v_old{l}"]
            put(f"vc{l}", vt)

    # the graph
    ctx = g.ggml_init(InitParams(8 << 20, None, True))
    gf = g.ggml_new_graph(ctx)
    scale = 1.0 / float(np.sqrt(D))
    rope = lambda x: g.ggml_rope_ext(ctx, x, leaves["pos"], None, D, 0, 8192, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
    q_in, outs = leaves["q"], []
    for l in range(LAYERS):
        kc, vc = leaves[f"kc{l}"], leaves[f"vc{l}"]
        q_cur, k_cur, v_cur = rope(q_in), rope(leaves[f"k{l}"]), leaves[f"v{l}"]
        for t in (q_cur, k_cur):
            g.ggml_build_forward_expand(gf, t)
        g.ggml_build_forward_expand(gf, g.ggml_cpy(ctx, k_cur, g.ggml_view_1d(ctx, kc, n * HK * D, ROW * j0)))
        v_view = g.ggml_view_2d(ctx, vc, n, HK * D, N_CTX * 2, j0 * 2)
        g.ggml_build_forward_expand(gf, g.ggml_cpy(ctx, g.ggml_transpose(ctx, v_cur), v_view))
        q = g.ggml_permute(ctx, q_cur, 0, 2, 1, 3)
        k = g.ggml_view_3d(ctx, kc, D, n_kv, HK, ROW, ROW // HK, 0)
        v = g.ggml_view_3d(ctx, vc, n_kv, D, HK, 2 * N_CTX, 2 * N_CTX * D, 0)
        kq = g.ggml_mul_mat(ctx, k, q)
        g.ggml_set_name(kq, f"kq-{l}".encode())
        kq = g.ggml_soft_max_ext(ctx, kq, leaves["mask"], scale, 0.0)
        kqv = g.ggml_mul_mat(ctx, v, kq)
        cur = g.ggml_cont_2d(ctx, g.ggml_permute(ctx, kqv, 0, 2, 1, 3), D * H, n)
        g.ggml_set_name(cur, f"kqv_out-{l}".encode())
        g.ggml_build_forward_expand(gf, cur)
        outs.append(cur)
        q_in = g.ggml_reshape_3d(ctx, cur, D, H, n)
    galloc = g.ggml_gallocr_new(g.ggml_backend_get_default_buffer_type(backend))
    assert g.ggml_gallocr_alloc_graph(galloc, gf)
    bad = []
    for i in range(g.ggml_graph_n_nodes(gf)):
        node = g.ggml_graph_node(gf, i)
        if not g.ggml_backend_supports_op(backend, node):
            bad.append(f"{g.ggml_op_desc(node).decode()}({g.ggml_get_name(node).decode()})")
    if bad:
        print("not supported by the backend:", ", ".join(bad), file=sys.stderr)
        sys.exit(3)
    st = g.ggml_backend_graph_compute(backend, gf)
    assert st == 0, f"graph_compute status {st}"

    res = {"out": np.empty((n, D * H), np.float32)}                      # (ggml-alloc has handed the first block's output buffer on: the last one's only)
    g.ggml_backend_tensor_get(outs[-1], res["out"].ctypes.data_as(C.c_void_p), 0, res["out"].nbytes)
    for l in range(LAYERS):
        kb = np.empty((n, ROW), np.uint8)
        g.ggml_backend_tensor_get(leaves[f"kc{l}"], kb.ctypes.data_as(C.c_void_p), ROW * j0, kb.nbytes)
        vt = np.empty((HK * D, N_CTX), np.float16)
        g.ggml_backend_tensor_get(leaves[f"vc{l}"], vt.ctypes.data_as(C.c_void_p), 0, vt.nbytes)
        res[f"k_rows{l}"], res[f"v_cache{l}"] = kb, vt
    np.savez(out_path, **res)
    g.ggml_gallocr_free(galloc)
    g.ggml_backend_buffer_free(buf_in)
    g.ggml_free(ctx)
    g.ggml_free(ctx_in)
    g.ggml_backend_free(backend)


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6])
