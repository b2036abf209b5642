"""CPU-side tests: the C-ABI library loads and exports every declared symbol (no compute without a GPU), the product
path fails loudly without a device, the workload tables match SURVEY.md's byte/flop accounting, and the row-split
partition + concat (the N > 1 path) is correct under a world_size-2 gloo run."""
import ctypes
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_capi_exports_every_declared_symbol():
    from ggml_hexagon_amd import build, capi
    so = build.build_qmm()
    lib = ctypes.CDLL(str(so))
    for hdr, exports in (("ggml_mi355x_qmm.h", capi.EXPORTS), ("ggml_mi355x_ops.h", capi.OPS_EXPORTS)):
        header = (ROOT / "include" / hdr).read_text()
        declared = re.findall(r"QMM_API\s+[\w\s\*]+?\b(qmm_\w+)\s*\(", header)
        assert len(declared) >= (20 if hdr.endswith("qmm.h") else 6)
        for name in declared:
            assert hasattr(lib, name), f"{name} declared in include/{hdr} but not exported"
        assert set(declared) == set(exports)
    assert lib.qmm_abi_version() == 2            # 2: chains, timing events, six more weight formats, Q8_1 activations
    lib.qmm_row_size.restype = ctypes.c_size_t
    lib.qmm_row_size.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert [lib.qmm_row_size(t, 4096) for t in (2, 8, 12, 13, 14)] == [2304, 4352, 2304, 2816, 3360]
    assert [lib.qmm_row_size(t, 4096) for t in (3, 6, 7, 10, 11, 20)] == [2560, 2816, 3072, 1344, 1760, 2304]     # SURVEY 8f-4 formats
    assert lib.qmm_row_size(12, 100) == 0 and lib.qmm_row_size(0, 4096) == 0


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    from ggml_hexagon_amd.capi import Qmm, QmmError
    with pytest.raises(QmmError):
        Qmm(0)


def test_plugin_module_exports_the_ggml_entry_points():
    so = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"
    if not so.exists():
        pytest.skip("plugin not built (needs the ggml headers of the host tree)")
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True).stdout
    for name in ("ggml_backend_init", "ggml_backend_score", "ggml_backend_mi355x_reg", "ggml_backend_mi355x_init",
                 "ggml_backend_is_mi355x", "ggml_backend_mi355x_get_device_count", "ggml_backend_mi355x_get_devname",
                 "ggml_backend_mi355x_buffer_type"):
        assert re.search(rf"\bT {name}\b", syms), name


def test_workload_accounting_matches_survey():
    from ggml_hexagon_amd import workload
    w = workload.get("synth-7b-q4_k")
    # 6,607,077,376 matmul weights x 0.5625 B = 3,716,481,024 B/token; pp512 = 6.766e12 flop
    assert w.weight_bytes() == 3_716_481_024
    assert w.flops(512) == 2 * 6_607_077_376 * 512
    assert len(w.all_mats()) == 32 * 7 + 1
    l3 = workload.get("llama3-8b-q4_k_m")
    types = {m.name: m.type for m in l3.all_mats()}
    assert types["blk.0.attn_v"] == 14 and types["blk.0.ffn_down"] == 14          # use_more_bits layers -> Q6_K
    assert types["blk.4.attn_v"] == 12 and types["blk.4.ffn_down"] == 12
    assert types["output"] == 14 and types["blk.7.attn_q"] == 12
    mx = workload.get("mixtral-8x7b-q4_k_m")
    ids = [m for m in mx.all_mats() if m.n_expert]
    assert len(ids) == 32 * 3 and ids[0].n_expert == 8 and ids[0].n_used == 2
    assert {m.type for m in mx.all_mats() if m.name.endswith("attn_k")} == {8}     # n_expert == 8: attn_k/v -> Q8_0
    l70 = workload.get("llama3-70b-q4_k_m")
    assert 13 in {m.type for m in l70.all_mats() if m.name.endswith("attn_v")}      # 70B rule: Q5_K


def test_row_ranges_follow_ggml_row_split():
    from ggml_hexagon_amd.rowsplit import ROW_ROUNDING, all_ranges, rounding_for, row_range
    assert ROW_ROUNDING == 256                               # the prefill kernels' row tile = the plugin's SPLIT_ROW_ROUNDING
    for m in (4096, 14336, 28672, 128256, 1024, 100):
        for world in (1, 2, 4, 8):
            rs = all_ranges(m, world)
            rnd = rounding_for(m, world)
            assert rs[0][0] == 0 and rs[-1][1] == m
            for (lo, hi), (lo2, _) in zip(rs, rs[1:]):
                assert hi == lo2 and lo % rnd == 0
            if m // world >= 32:                             # no rank left without rows where 32-row slices exist (1024 rows on 8 ranks)
                assert all(hi > lo for lo, hi in rs), (m, world, rs)
    assert rounding_for(1024, 8) == 128 and rounding_for(8192, 8) == 256 and rounding_for(1024, 2) == 256
    assert all_ranges(1024, 8) == [(128 * i, 128 * i + 128) for i in range(8)]
    # cumulative fractions rounded DOWN to the rounding, the last device takes the remainder (ggml-cuda.cu:740-753)
    assert row_range(128256, 7, 8) == (112128, 128256)
    assert row_range(128256, 7, 8, rounding=64) == (112192, 128256)
    assert all_ranges(100, 4, rounding=64) == [(0, 0), (0, 0), (0, 64), (64, 100)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rowsplit_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ggml_hexagon_amd import rowsplit, synth
        from oracle.pyoracle import Oracle
        o = Oracle()
        cc = rowsplit.RowConcat()
        ok = True
        for (t, m, k, n) in ((12, 256, 512, 3), (14, 200, 256, 1), (2, 192, 64, 5)):
            w = synth.synth_weights(t, m, k, seed=3, sigma=0.2)                 # every rank builds the full matrix ...
            x = np.random.default_rng(1).uniform(-1, 1, (n, k)).astype(np.float32)
            ranges = rowsplit.all_ranges(m, world)
            lo, hi = ranges[rank]
            local = o.mul_mat(t, w[lo:hi], k, x) if hi > lo else np.zeros((n, 0), np.float32)   # ... computes only its rows
            full = cc.concat(torch.from_numpy(np.ascontiguousarray(local)), ranges).numpy()
            ok &= np.array_equal(full, o.mul_mat(t, w, k, x))                   # concat == single-device result, bit for bit
        q.put((rank, bool(ok)))
    except Exception as e:                                                      # report instead of hanging the parent
        q.put((rank, f"{type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


def test_rowsplit_concat_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rowsplit_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)]


# ---- the bench driver's multi-GPU path (HotPath + RowConcat) on CPU tensors, world_size 2, gloo, with the kernels replaced
#      by the oracle (allowed here: tests may use the oracle as the checker/stand-in; the product path never does)

class _OracleQmm:
    """same method surface as capi.Qmm, computing with oracle/qmm_oracle.c on CPU tensors"""

    def __init__(self):
        from oracle.pyoracle import Oracle
        self.o = Oracle()

    def planar_type(self, t, k, row_bytes):      # the CPU stand-in keeps GGUF wire layout (the planar repack is a device matter)
        return 0

    def mul_mat_group(self, weights, k, x, outs):
        import torch
        for (t, w), out in zip(weights, outs):
            out.copy_(torch.from_numpy(self.o.mul_mat(t, w.numpy(), k, x.numpy())))
        return outs


def _hotpath_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ggml_hexagon_amd import rowsplit, synth, workload
        from ggml_hexagon_amd.hotpath import HotPath
        # a 2-layer toy model with the real per-layer structure (grouped q/k/v with mixed types, gate/up, down, output)
        wl = workload._llama("toy", 2, 256, 512, 4, 2, 1000, "q4_k_m")
        orig = synth.synth_weights_torch
        synth.synth_weights_torch = lambda t, rows, k, device, seed=0, sigma=0.02: torch.from_numpy(synth.synth_weights(t, rows, k, seed=seed, sigma=0.2))
        try:
            qm = _OracleQmm()
            hp = HotPath(qm, wl, torch.device("cpu"), rank, world, rowsplit.RowConcat(), seed=5)
            for n, n_out in ((1, None), (3, None), (3, 1)):      # (3, 1): a prompt batch that wants one row of logits
                if n_out is not None:
                    for t in hp.prepare(n_out)[2].values():      # stale results of the n = 1 pass must not satisfy the check
                        t.zero_()
                hp.run(n, n_out)
                # every full dst must equal the single-device product of the concatenated shards
                assert any(isinstance(k, tuple) and k and k[0] == "group" for k in hp.prepare(n)[1]), "grouped exchange not in use"
                for grp in wl.groups[-5:]:                       # the last layer (q/k/v and gate/up travel as ONE all-gather each) + the output projection (ragged split)
                    nn = n_out if (n_out is not None and grp.outputs_only) else n     # the last layer's FFN and the output projection ran at n_outputs
                    x, dst_local, dst_full, _ = hp.prepare(nn)
                    for m in grp.mats:
                        w_local, ranges = hp.weights[m.name]
                        gathered = [None] * world
                        dist.all_gather_object(gathered, w_local.numpy())
                        w_full = np.concatenate([g for g in gathered if g.shape[0] > 0])
                        want = qm.o.mul_mat(m.type, w_full, m.K, x[m.K].numpy())
                        got = dst_full[(m.name.split(".")[-1], w_local.shape[0])].numpy()
                        assert got.shape == want.shape and np.array_equal(got, want), (m.name, n, n_out)
            q.put((rank, True))
        finally:
            synth.synth_weights_torch = orig
    except Exception as e:
        import traceback
        q.put((rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()[-800:]}"))
    finally:
        dist.destroy_process_group()


def test_hotpath_rowsplit_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_hotpath_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)], res


def test_bench_dump_outputs_writes_what_the_passes_computed(tmp_path, monkeypatch):
    """bench.py --dump-outputs on the CPU stand-in: every dst buffer the timed passes write and none they leave alone (the prompt
    batch's output projection when one row wants logits), prompt-batch buffers cut to the same seeded rows, float32, under the
    64 MB cap, and the same files from two runs on the same seeds"""
    import torch
    import bench
    from ggml_hexagon_amd import synth, workload
    from ggml_hexagon_amd.hotpath import HotPath
    monkeypatch.setattr(synth, "synth_weights_torch", lambda t, rows, k, device, seed=0, sigma=0.02:
                        torch.from_numpy(synth.synth_weights(t, rows, k, seed=seed, sigma=0.2)))
    wl = workload._llama("toy", 2, 256, 512, 4, 2, 1000, "q4_k_m")
    dumps = []
    for run in range(2):
        hp = HotPath(_OracleQmm(), wl, torch.device("cpu"), seed=5)
        hp.run(100, 1)                      # a prompt batch that wants one row of logits, then a token
        hp.run(1)
        bench.dump_outputs(hp, tmp_path / str(run), 100, 1, 1)
        dumps.append({f.name: np.load(f) for f in sorted((tmp_path / str(run)).iterdir())})
    a, b = dumps
    names = ("attn_q_256", "attn_k_128", "attn_v_128", "attn_output_256", "ffn_gate_512", "ffn_up_512", "ffn_down_256")
    assert set(a) == {f"pp100_{n}.npy" for n in names} | {f"tg_{n}.npy" for n in names + ("output_1000",)}
    rows = np.sort(np.random.default_rng(0).choice(100, bench.DUMP_ROWS, replace=False))
    _, pp_dst, _, _ = hp.io[100]
    _, tg_dst, _, _ = hp.io[1]
    for name, arr in a.items():
        assert arr.dtype == np.float32 and np.array_equal(arr, b[name]), name
        stage, rest = name[:-4].split("_", 1)
        key = (rest.rsplit("_", 1)[0], int(rest.rsplit("_", 1)[1]))
        want = pp_dst[key].numpy()[rows] if stage == "pp100" else tg_dst[key].numpy()
        assert np.array_equal(arr, want), name
    assert sum(arr.nbytes for arr in a.values()) <= bench.DUMP_MAX_BYTES


def test_prompt_pass_counts_output_rows_only():
    """llama-bench's prompt test wants one row of logits: the last layer's FFN and the output projection run at
    n_outputs = 1 (workload.Group.outputs_only), everything else at n_prompt"""
    from ggml_hexagon_amd import workload
    wl = workload.get("llama3-8b-q4_k_m")
    only = [g for g in wl.groups if g.outputs_only]
    assert [m.name for g in only for m in g.mats] == ["blk.31.ffn_gate", "blk.31.ffn_up", "blk.31.ffn_down", "output"]
    full, bench = wl.flops(512), wl.flops(512, 1)
    saved = sum(m.flops(512) - m.flops(1) for g in only for m in g.mats)
    assert full - bench == saved and 0.05 < saved / full < 0.12
    assert wl.flops(1, 1) == wl.flops(1) and wl.algo_bytes(1, 1) == wl.algo_bytes(1)          # token generation is unchanged


def test_glue_op_surface_predicates():
    """qmm_op_supported is pure host logic (no device needed): the surface the plugin's supports_op reports.  Shapes follow
    llama.cpp's layer graph (src/llama-model.cpp:4191-4350, src/llama-graph.cpp:1126-1213)."""
    from ggml_hexagon_amd import build, capi
    from ggml_hexagon_amd.capi import QmmTensor as T
    lib = ctypes.CDLL(str(build.build_qmm()))
    P = ctypes.POINTER(capi.QmmTensor)
    lib.qmm_op_supported.argtypes = [ctypes.c_int, P, P, P, P]
    lib.qmm_attn_decode_supported.argtypes = [P, P, P, P, P]
    lib.qmm_op_add_rms_norm_supported.argtypes = [P, P, P, P, P]

    def sup(op, a, b, c, d):
        r = lambda t: ctypes.byref(t) if t is not None else None
        return lib.qmm_op_supported(op, r(a), r(b), r(c), r(d))

    F32, F16, I32, BF16, Q4K = 0, 1, 26, 30, 12
    x = T.make(F32, [4096, 512])
    w = T.make(F32, [4096])
    assert sup(capi.OP_RMS_NORM, x, None, None, x) == 1
    assert sup(capi.OP_RMS_NORM_MUL, x, w, None, x) == 1
    assert sup(capi.OP_RMS_NORM, T.make(F16, [4096, 512]), None, None, T.make(F16, [4096, 512])) == 0
    assert sup(capi.OP_ADD, x, x, None, x) == 1 and sup(capi.OP_MUL, x, w, None, x) == 1          # broadcast row
    assert sup(capi.OP_ADD, x, T.make(F32, [4095]), None, x) == 0                                   # not repeatable
    assert sup(capi.OP_SILU_MUL, x, x, None, x) == 1
    # rope: normal and neox yes, m-rope / vision no; positions must be i32 of ne2 entries
    q = T.make(F32, [128, 32, 512])
    pos = T.make(I32, [512])
    rope = lambda mode: T.make(F32, [128, 32, 512], op_params=[0, 128, mode, 0, 8192])
    assert sup(capi.OP_ROPE, q, pos, None, rope(0)) == 1 and sup(capi.OP_ROPE, q, pos, None, rope(2)) == 1
    assert sup(capi.OP_ROPE, q, pos, None, rope(8)) == 0 and sup(capi.OP_ROPE, q, pos, None, rope(24)) == 0
    assert sup(capi.OP_ROPE, q, T.make(I32, [511]), None, rope(0)) == 0
    # soft_max with an f32 or f16 mask of at least ne01 rows
    kq = T.make(F32, [640, 512, 32])
    assert sup(capi.OP_SOFT_MAX, kq, T.make(F32, [640, 512]), None, kq) == 1
    assert sup(capi.OP_SOFT_MAX, kq, T.make(F16, [640, 512]), None, kq) == 1
    assert sup(capi.OP_SOFT_MAX, kq, T.make(F32, [640, 256]), None, kq) == 0
    # cpy: f32 <-> f16 any strides, no bf16 / quantized destinations
    assert sup(capi.OP_CPY, x, None, None, T.make(F16, [4096, 512])) == 1
    assert sup(capi.OP_CPY, x, None, None, T.make(BF16, [4096, 512])) == 0
    assert sup(capi.OP_CPY, x, None, None, T.make(Q4K, [4096, 512])) == 0
    # get_rows from a quantized embedding table
    emb = T.make(Q4K, [4096, 32000], nb=[144, 2304, 2304 * 32000, 2304 * 32000])
    assert sup(capi.OP_GET_ROWS, emb, T.make(I32, [512]), None, x) == 1
    # KQ: K is a strided view of the f16 cache, Q a permuted f32 tensor; grouped-query broadcast 32 / 8
    k = T.make(F16, [128, 640, 8], nb=[2, 2048, 256, 2048 * 640])
    qp = T.make(F32, [128, 512, 32], nb=[4, 16384, 512, 16384 * 512])
    assert sup(capi.OP_MUL_MAT_F, k, qp, None, T.make(F32, [640, 512, 32])) == 1
    assert sup(capi.OP_MUL_MAT_F, T.make(F16, [128, 640, 8], nb=[2048, 2, 256, 1]), qp, None, T.make(F32, [640, 512, 32])) == 0   # K not dense along D
    # the fused forms
    r = ctypes.byref
    assert lib.qmm_op_add_rms_norm_supported(r(x), r(x), r(w), r(x), r(x)) == 1
    assert lib.qmm_op_add_rms_norm_supported(r(x), r(w), r(w), r(x), r(x)) == 0                   # broadcast add is not the residual add
    q1 = T.make(F32, [128, 1, 32], nb=[4, 16384, 512, 16384])
    v = T.make(F16, [640, 128, 8], nb=[2, 1280, 1280 * 128, 1280 * 1024])
    m1 = T.make(F32, [640, 64])
    out = T.make(F32, [4096, 1])
    assert lib.qmm_attn_decode_supported(r(q1), r(k), r(v), r(m1), r(out)) == 1
    assert lib.qmm_attn_decode_supported(r(qp), r(k), r(v), r(T.make(F32, [640, 512])), r(T.make(F32, [4096, 512]))) == 0      # prefill batch


# ---- the switch table (csrc/qmm_switches.h): the one list of GGML_MI355X_* environment switches

SWITCH_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_switches.h"
# name -> (kind, value with the variable unset), read off qmm_create, qmm_ops.hip, qmm_comm.hip and the plugin as they were before the
# table existed.  STR switches have no number: None.  SKINNY_MAXN 0 = the built-in bounds (64, and 128 for matrices with few row
# groups); CHAIN 0 is the plugin's default (the library's qmm_chain_begin records unless CHAIN=0 is set: test_gpu_chain.py).
SWITCH_DEFAULTS = {
    "PREC": ("STR", None), "ACT_MODE": ("ATOI", 0), "SPLITK": ("ATOI", 1), "SPLITK_COMBINE": ("ATOI", 0), "SKINNY": ("ATOI", 1),
    "SKINNY_MAXN": ("ATOI", 0), "MM_GROUP": ("ATOI", 1), "MV_KMIX": ("ATOI", 2), "MV_BPC": ("ATOI", 1), "MV_ONEPASS": ("ATOI", 1),
    "REGB_Q23": ("ATOI", 1), "WIDE": ("ATOI", 1), "R64": ("ATOI", 2), "R64S": ("ATOI", 1), "PREP_REG": ("ATOI", 1),
    "ABLATE": ("ATOI", 0), "ATTN_SHORT": ("OFF0", 1), "ATTN_SPLIT": ("OFF0", 1), "RCCL_LIB": ("STR", None), "CHAIN": ("ATOI", 0),
    "GLUE": ("OFF0", 1), "FUSE": ("OFF0", 1), "ATTN_ROPE": ("OFF0", 1), "REPACK": ("OFF0", 1), "STAGED_SET": ("OFF0", 1),
    "RCCL": ("ATOI", 0), "TIMING": ("ATOI", 0), "NO_PINNED": ("PRESENT", 0), "DEBUG": ("PRESENT", 0), "VIRTUAL_DEVICES": ("STR", None),
    "ROUTER_NORM_OFF": ("PRESENT", 0), "PREP_NORM_OFF": ("PRESENT", 0), "ROUTER_LOGITS_OFF": ("PRESENT", 0),
    "MOE_SWIGLU_OFF": ("PRESENT", 0), "MOE_COMBINE_NORM_OFF": ("PRESENT", 0),
}
SWITCH_PROBE = r"""
#include "qmm_switches.h"
#include <cstdio>
int main(int argc, char **) {
    using namespace qmm_sw;
    static const char * kinds[] = { "ATOI", "OFF0", "PRESENT", "STR" };
    const values v = read();
    for (int i = 0; i < SW_COUNT; ++i) {
        if (argc > 1) printf("%s %s %d\n", table[i].name, kinds[table[i].k], table[i].def);
        else printf("%s %d %d %s\n", table[i].name, v[(id) i], (int) v.is_set((id) i), v.str((id) i) ? v.str((id) i) : "(null)");
    }
    if (argc == 1) printf("prec_is_bf16 %d\n", (int) prec_is_bf16(v.str(SW_PREC)));
    return 0;
}
"""


@pytest.fixture(scope="module")
def switch_probe(tmp_path_factory):
    """the header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the table / one reading of the environment"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("switches")
    (d / "probe.cpp").write_text(SWITCH_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{SWITCH_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(env=None, table=False):
        base = {k: v for k, v in os.environ.items() if not k.startswith("GGML_MI355X_")}
        out = subprocess.run([str(d / "probe")] + (["table"] if table else []), env=dict(base, **{f"GGML_MI355X_{k}": v for k, v in (env or {}).items()}),
                             check=True, capture_output=True, text=True).stdout
        return {l.split()[0].replace("GGML_MI355X_", ""): l.split()[1:] for l in out.splitlines()}
    return run


def test_switch_table_keeps_every_name_kind_and_default(switch_probe):
    table = switch_probe(table=True)
    assert len(table) == 35 and set(table) == set(SWITCH_DEFAULTS)
    unset = switch_probe()
    for name, (kind, default) in SWITCH_DEFAULTS.items():
        assert table[name][0] == kind, name
        assert unset[name][1:] == ["0", "(null)"], name                  # not set, no text
        if kind != "STR":
            assert int(unset[name][0]) == default, name
            assert int(table[name][1]) == default, name
    assert unset["prec_is_bf16"] == ["0"]                                  # f16 on Q8 activations unless asked


def test_switch_parse_rules(switch_probe):
    val = lambda env, name: int(switch_probe(env)[name][0])
    # value by atoi
    assert val({"R64": "3"}, "R64") == 3 and val({"SPLITK": "0"}, "SPLITK") == 0 and val({"TIMING": "1"}, "TIMING") == 1
    assert val({"MV_KMIX": "junk"}, "MV_KMIX") == 0                                              # atoi of no number
    # off only when set to 0
    for name in ("ATTN_SHORT", "ATTN_SPLIT", "GLUE", "FUSE", "ATTN_ROPE", "REPACK", "STAGED_SET"):
        assert val({name: "0"}, name) == 0 and val({name: "1"}, name) == 1 and val({name: "2"}, name) == 1, name
        assert val({name: ""}, name) == 0 and val({name: "off"}, name) == 0, name               # atoi == 0
    # on by mere presence, "0" included
    for name in ("DEBUG", "NO_PINNED", "ROUTER_NORM_OFF", "PREP_NORM_OFF", "ROUTER_LOGITS_OFF", "MOE_SWIGLU_OFF", "MOE_COMBINE_NORM_OFF"):
        assert val({name: "1"}, name) == 1 and val({name: "0"}, name) == 1 and val({name: ""}, name) == 1, name
    # validity: MV_BPC only in 1..8, SKINNY_MAXN only from 9 up; anything else leaves the default
    assert [val({"MV_BPC": v}, "MV_BPC") for v in ("0", "1", "4", "8", "9", "-2")] == [1, 1, 4, 8, 1, 1]
    assert [val({"SKINNY_MAXN": v}, "SKINNY_MAXN") for v in ("8", "9", "96", "0", "-1")] == [0, 9, 96, 0, 0]
    # strings: the text as it is; PREC is bf16 for "bf16" or "0" and f16 on Q8 for anything else
    r = switch_probe({"PREC": "bf16", "RCCL_LIB": "/x/librccl.so", "VIRTUAL_DEVICES": "2"})
    assert r["PREC"][1:] == ["1", "bf16"] and r["RCCL_LIB"][2] == "/x/librccl.so" and r["VIRTUAL_DEVICES"][2] == "2"
    assert [switch_probe({"PREC": v})["prec_is_bf16"] for v in ("bf16", "0", "f16q8", "1", "BF16", "")] == [["1"], ["1"], ["0"], ["0"], ["0"], ["0"]]
    # a switch that is set reports it (the library's CHAIN and ABLATE act only then)
    assert switch_probe({"CHAIN": "0"})["CHAIN"][:2] == ["0", "1"] and switch_probe({"ABLATE": "5"})["ABLATE"][:2] == ["5", "1"]


def test_every_switch_is_documented():
    text = (ROOT / "INTEGRATION.md").read_text()
    for name in SWITCH_DEFAULTS:
        assert re.search(rf"`GGML_MI355X_{name}\b", text), f"GGML_MI355X_{name} is not in INTEGRATION.md"


def test_switch_names_live_in_the_header_only():
    """no GGML_MI355X_* environment name as a string literal anywhere else in csrc/ (comments may speak of them; the public macros
    GGML_MI355X_BACKEND_NAME / _MAX_DEVICES are not strings), and no getenv outside the header"""
    for f in sorted((ROOT / "ggml-hexagon_amd" / "csrc").iterdir()):
        if f == SWITCH_HEADER or f.suffix not in (".cpp", ".h", ".hip", ".hiph"):
            continue
        for n, line in enumerate(f.read_text().splitlines(), 1):
            code = re.sub(r"//.*$", "", line)
            assert not re.search(r'"(?:[^"\\]|\\.)*GGML_MI355X_', code), f"{f.name}:{n}: {line.strip()[:120]}"
            assert "getenv" not in code, f"{f.name}:{n}: {line.strip()[:120]}"


# ---- the prefill launch plan (csrc/qmm_prefill_plan.h): kernel, tile, split-K, activation prep, key and workspace of a prefill run

PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_prefill_plan.h"
PLAN_PROBE = r"""
#include "qmm_prefill_plan.h"
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
static void line(const PrefillPlan & p) {
    printf("%s%s grid=%u,%u,%u block=%u lds=%zu ksplit=%d frag=%d prep=%s perm=%d key=%d ws=%zu", p.label, p.combine_ok ? "+combine" : "", p.grid[0], p.grid[1],
           p.grid[2], p.block, p.lds, p.ksplit, p.frag_major, p.prep_label, p.perm, p.key, p.ws_total);
}
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {          // cus type M1,M2,.. K N n_expert flags [NAME=VAL ...]
        std::istringstream in(spec);
        PrefillRules r = { 256, QMM_PREC_F16_Q8, 1, 64, 128, 1, 0, 1 << 16, 1, 2, 1, 1, 1, 1 };      // qmm_ctx's defaults
        int type, ne; unsigned flags; int64_t K, N, M[4]; std::string ms, kv;
        in >> r.cus >> type >> ms >> K >> N >> ne >> flags;
        int n = 0;
        { std::istringstream m(ms); std::string x; while (std::getline(m, x, ',')) M[n++] = atoll(x.c_str()); }
        while (in >> kv) {
            const std::string name = kv.substr(0, kv.find('=')); const int v = atoi(kv.c_str() + kv.find('=') + 1);
            if (name == "R64") r.r64 = v; else if (name == "SPLITK") r.splitk = v; else if (name == "SKINNY") r.skinny = v;
            else if (name == "SKINNY_MAXN") r.skinny_max_n = r.skinny_max_n_few = v; else if (name == "WIDE") r.wide = v; else if (name == "R64S") r.r64s = v;
            else if (name == "PREP_REG") r.prep_reg = v; else if (name == "REGB_Q23") r.regb_q23 = v; else if (name == "MM_GROUP") r.mm_group = v;
            else if (name == "SPLITK_COMBINE") r.splitk_combine = v; else if (name == "BF16") r.prec = v ? QMM_PREC_BF16 : QMM_PREC_F16_Q8; else return 1;
        }
        const PrefillPlan p = prefill_plan(r, type, M, n, K, N, ne, flags);
        if (p.per_matrix) {
            printf("per_matrix");
            for (int i = 0; i < n; ++i) { printf("; "); line(prefill_plan(r, type, M + i, 1, K, N, 1, flags)); }
        } else line(p);
        printf("\n");
    }
    return 0;
}
"""
# (run, what the launch code did with it before the plan existed).  A run: CUs, weight type id, the rows of its 1..4 matrices, K, tokens
# (MUL_MAT_ID: (token, slot) pairs), n_expert, flags (1 = MUL_MAT_ID, 2 = SwiGLU input, 4 = fused norm), switches off their defaults.
# The right-hand sides were printed by the decision functions of the commit before this header (mfma_use_skinny, mfma_use_wide, mfma_splitk,
# mfma_prep_key, launch_prep, launch_mfma, launch_mfma_regb_t, mfma_mul_mat, mfma_mul_mat_group, moe_mul_mat_id) copied into a stand-alone
# program, never by the header: every distinct matrix of the five BASELINE workloads at 512 tokens, the few-token kernel's bounds, MoE, other
# chip sizes, and each prefill switch off its default.  "per_matrix": the run is one launch per matrix, listed behind it.
PLAN_TABLE = [
    ("256 2 4096,4096,4096 4096 512 1 0",
     "per_matrix; mfma_regb_kernel<2,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_kernel<8> perm=4 key=6 ws=37751040; mfma_regb_kernel<2,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_kernel<8> perm=4 key=6 ws=37751040; mfma_regb_kernel<2,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_kernel<8> perm=4 key=6 ws=37751040"),
    ("256 2 4096 4096 512 1 0",
     "mfma_regb_kernel<2,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_kernel<8> perm=4 key=6 ws=37751040"),
    ("256 2 11008,11008 4096 512 1 0",
     "mfma_regb_kernel<2,8,128> grid=86,4,1 block=512 lds=32768 ksplit=1 frag=0 prep=prep_act_kernel<8> perm=4 key=6 ws=4196608"),
    ("256 2 4096 11008 512 1 2",
     "mfma_regb_kernel<2,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_kernel<8> perm=4 key=6 ws=44828928"),
    ("256 14 32000 4096 512 1 0",
     "mfma_regb_kernel<14,8,128> grid=125,4,1 block=512 lds=65536 ksplit=1 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=4196608"),
    ("256 12 4096,1024,1024 4096 512 1 0",
     "mfma_regb_kernel<12,8,128> grid=24,4,2 block=512 lds=32768 ksplit=2 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=29362432"),
    ("256 12 4096,1024 4096 512 1 0",
     "mfma_regb_kernel<12,8,128> grid=20,4,3 block=512 lds=32768 ksplit=3 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=35653888"),
    ("256 14 1024 4096 512 1 0",
     "mfma_regb_kernel<14,8,128> grid=4,4,8 block=512 lds=65536 ksplit=8 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=20973824"),
    ("256 12 4096 4096 512 1 0",
     "mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040"),
    ("256 12 14336,14336 4096 512 1 0",
     "mfma_r64s_q4k_kernel<2> grid=112,2,1 block=256 lds=0 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 4096 14336 512 1 2",
     "mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=48236800"),
    ("256 14 4096 14336 512 1 2",
     "mfma_regb_kernel<14,8,128> grid=16,4,4 block=512 lds=65536 ksplit=4 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=48236800"),
    ("256 14 128256 4096 512 1 0",
     "mfma_regb_kernel<14,8,128> grid=501,4,1 block=512 lds=65536 ksplit=1 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=4196608"),
    ("256 12 8192,1024 8192 512 1 0",
     "per_matrix; mfma_regb_kernel<12,8,128> grid=32,4,2 block=512 lds=32768 ksplit=2 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=41945344; mfma_regb_kernel<12,8,128> grid=4,4,8 block=512 lds=32768 ksplit=8 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=25168128"),
    ("256 13 1024 8192 512 1 0",
     "mfma_regb_kernel<13,8,128> grid=4,4,8 block=512 lds=32768 ksplit=8 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=25168128"),
    ("256 14 1024 8192 512 1 0",
     "mfma_regb_kernel<14,8,128> grid=4,4,8 block=512 lds=65536 ksplit=8 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=25168128"),
    ("256 12 8192 8192 512 1 0",
     "mfma_regb_kernel<12,8,128> grid=32,4,2 block=512 lds=32768 ksplit=2 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=41945344"),
    ("256 12 28672,28672 8192 512 1 0",
     "mfma_r64s_q4k_kernel<2> grid=224,2,1 block=256 lds=0 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=8390912"),
    ("256 12 8192 28672 512 1 2",
     "mfma_regb_kernel<12,8,128> grid=32,4,2 block=512 lds=32768 ksplit=2 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=62916864"),
    ("256 14 8192 28672 512 1 2",
     "mfma_regb_kernel<14,8,128> grid=32,4,2 block=512 lds=65536 ksplit=2 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=62916864"),
    ("256 14 128256 8192 512 1 0",
     "mfma_regb_kernel<14,8,128> grid=501,4,1 block=512 lds=65536 ksplit=1 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=8390912"),
    ("256 12 4096 4096 512 1 0",
     "mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040"),
    ("256 8 1024,1024 4096 512 1 0",
     "mfma_regb_kernel<8,8,128> grid=8,4,8 block=512 lds=32768 ksplit=8 frag=0 prep=prep_act_kernel<8> perm=5 key=18 ws=37751040"),
    ("256 13 4096 4096 512 1 0",
     "mfma_regb_kernel<13,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040"),
    ("256 12 14336 4096 1024 8 1",
     "mfma_regb_kernel<12,8,128> grid=56,8,8 block=512 lds=32768 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=0 ws=9458944"),
    ("256 12 4096 14336 1024 8 1",
     "mfma_regb_kernel<12,8,128> grid=16,8,8 block=512 lds=32768 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=0 ws=33051904"),
    ("256 14 4096 14336 1024 8 1",
     "mfma_regb_kernel<14,8,128> grid=16,8,8 block=512 lds=65536 ksplit=1 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=0 ws=33051904"),
    ("256 14 32000 4096 512 1 0",
     "mfma_regb_kernel<14,8,128> grid=125,4,1 block=512 lds=65536 ksplit=1 frag=0 prep=prep_act_q8k_kernel<3> perm=3 key=26 ws=4196608"),
    ("256 12 4096,4096,4096 4096 512 1 0",
     "per_matrix; mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040; mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040; mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040"),
    ("256 12 11008,11008 4096 512 1 0",
     "mfma_regb_kernel<12,8,128> grid=86,4,1 block=512 lds=32768 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 4096 11008 512 1 2",
     "mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_kernel<15> perm=2 key=26 ws=44828928"),
    ("256 12 32000 4096 512 1 0",
     "mfma_r64s_q4k_kernel<2> grid=125,2,1 block=256 lds=0 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 4096 4096 64 1 0",
     "mfma_skinny_kernel<12,8,2> grid=128,1,1 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=27 ws=1049344"),
    ("256 12 4096 4096 65 1 0",
     "mfma_skinny_kernel<12,8,2> grid=128,2,1 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=27 ws=1049344"),
    ("256 12 14336 4096 65 1 0",
     "mfma_regb_kernel<12,8,128> grid=56,1,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=15958784"),
    ("256 12 4096 4096 128 1 0",
     "mfma_skinny_kernel<12,8,2> grid=128,2,1 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=27 ws=1049344"),
    ("256 12 4096 4096 129 1 0",
     "mfma_regb_kernel<12,8,128> grid=16,2,8 block=512 lds=32768 ksplit=8 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=19006720"),
    ("256 12 4096,1024,1024 4096 128 1 0",
     "per_matrix; mfma_skinny_kernel<12,8,2> grid=128,2,1 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=27 ws=1049344; mfma_skinny_kernel<12,8,2> grid=32,2,1 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=27 ws=1049344; mfma_skinny_kernel<12,8,2> grid=32,2,1 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=27 ws=1049344"),
    ("256 12 4096,1024,1024 4096 512 1 4",
     "mfma_regb_kernel<12,8,128> grid=24,4,2 block=512 lds=32768 ksplit=2 frag=0 prep=prep_act_q8k_kernel<2,norm> perm=2 key=26 ws=29362432"),
    ("256 12 14336 4096 64 8 1",
     "mfma_skinny_kernel<12,8,2> grid=448,1,8 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=0 ws=1575424"),
    ("304 12 4096,1024,1024 4096 512 1 0",
     "mfma_regb_kernel<12,8,128> grid=24,4,3 block=512 lds=32768 ksplit=3 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=41945344"),
    ("64 12 14336,14336 4096 512 1 0",
     "mfma_r64s_q4k_kernel<2> grid=112,2,1 block=256 lds=0 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 14336,14336 4096 512 1 0 R64=0",
     "mfma_regb_q4k_wide_kernel<8> grid=112,2,1 block=512 lds=65536 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 4096 4096 512 1 0 R64=1",
     "mfma_r64_q4k_kernel<4> grid=16,4,4 block=256 lds=0 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040"),
    ("256 12 14336,14336 4096 512 1 0 R64=3",
     "mfma_r64s_q4k_kernel<2> grid=112,2,1 block=256 lds=0 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 14336,14336 4096 512 1 0 R64S=0",
     "mfma_r64_q4k_kernel<8> grid=112,2,1 block=256 lds=0 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 14336,14336 4096 512 1 0 WIDE=0",
     "mfma_regb_kernel<12,8,128> grid=112,4,1 block=512 lds=32768 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 4096 4096 512 1 0 SPLITK=0",
     "mfma_regb_kernel<12,4,64> grid=32,8,1 block=256 lds=16384 ksplit=1 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=4196608"),
    ("256 12 4096,1024,1024 4096 512 1 0 SPLITK=2",
     "mfma_regb_kernel<12,8,128> grid=24,4,2 block=512 lds=32768 ksplit=2 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=29362432"),
    ("256 12 4096 4096 512 1 0 SPLITK_COMBINE=1",
     "mfma_regb_kernel<12,8,128>+combine grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040"),
    ("256 12 4096 4096 32 1 0 SKINNY=0",
     "mfma_regb_kernel<12,8,128> grid=16,1,8 block=512 lds=32768 ksplit=8 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=5243648"),
    ("256 12 4096 4096 96 1 0 SKINNY_MAXN=96",
     "mfma_skinny_kernel<12,8,2> grid=128,2,1 block=512 lds=0 ksplit=1 frag=1 prep=prep_act_q8k_kernel<2> perm=2 key=27 ws=1049344"),
    ("256 12 4096,1024,1024 4096 512 1 0 MM_GROUP=0",
     "per_matrix; mfma_regb_kernel<12,8,128> grid=16,4,4 block=512 lds=32768 ksplit=4 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=37751040; mfma_regb_kernel<12,8,128> grid=4,4,8 block=512 lds=32768 ksplit=8 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=20973824; mfma_regb_kernel<12,8,128> grid=4,4,8 block=512 lds=32768 ksplit=8 frag=0 prep=prep_act_q8k_kernel<2> perm=2 key=26 ws=20973824"),
    ("256 14 4096 14336 512 1 0 PREP_REG=0",
     "mfma_regb_kernel<14,8,128> grid=16,4,4 block=512 lds=65536 ksplit=4 frag=0 prep=prep_act_kernel<15> perm=3 key=26 ws=48236800"),
    ("256 11 4096,1024 4096 512 1 0 REGB_Q23=0",
     "per_matrix; mfma_kernel<11,64> grid=64,4,1 block=512 lds=98304 ksplit=1 frag=0 prep=prep_act_q8k_kernel<0> perm=0 key=24 ws=4196608; mfma_kernel<11,64> grid=16,4,1 block=512 lds=98304 ksplit=1 frag=0 prep=prep_act_q8k_kernel<0> perm=0 key=24 ws=4196608"),
    ("256 14 4096 4096 512 1 0 BF16=1",
     "mfma_kernel<14,64> grid=64,4,1 block=512 lds=98304 ksplit=1 frag=0 prep=prep_act_kernel<15> perm=0 key=0 ws=4196608"),
]


@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each run on its input"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("plan")
    (d / "probe.cpp").write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_prefill_plan_keeps_every_decision(plan_probe):
    assert len(PLAN_TABLE) >= 40
    got = plan_probe([spec for spec, _ in PLAN_TABLE])
    assert len(got) == len(PLAN_TABLE)
    for (spec, want), line in zip(PLAN_TABLE, got):
        assert line == want, spec


def test_prefill_rules_live_in_the_plan_header_only():
    """the decision functions are the plan's own: no other file in csrc/ calls or defines them (comments may speak of them)"""
    for f in sorted((ROOT / "ggml-hexagon_amd" / "csrc").iterdir()):
        if f == PLAN_HEADER or f.suffix not in (".cpp", ".h", ".hip", ".hiph"):
            continue
        for n, line in enumerate(f.read_text().splitlines(), 1):
            code = re.sub(r"//.*$", "", line)
            assert not re.search(r"\b(mfma_use_skinny|mfma_use_wide|mfma_splitk)\b", code), f"{f.name}:{n}: {line.strip()[:120]}"


# ---- the group plan (prefill_group_plan of the same header): the launches of a whole qmm_mul_mat_group call at a prompt batch

GROUP_PROBE = r"""
#include "qmm_prefill_plan.h"
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
using namespace qmm;
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {          // cus type1,type2,.. M1,M2,.. K N flags [NAME=VAL ...]
        std::istringstream in(spec);
        PrefillRules r = { 256, QMM_PREC_F16_Q8, 1, 64, 128, 1, 0, 1 << 16, 1, 2, 1, 1, 1, 1 };      // qmm_ctx's defaults
        unsigned flags; int64_t K, N; std::string ts, ms, kv;
        in >> r.cus >> ts >> ms >> K >> N >> flags;
        std::vector<qmm_weight> ws;
        { std::istringstream t(ts), m(ms); std::string x, y;
          while (std::getline(t, x, ',') && std::getline(m, y, ',')) { qmm_weight w = {}; w.type = atoi(x.c_str()); w.M = atoll(y.c_str()); ws.push_back(w); } }
        while (in >> kv) {
            const std::string name = kv.substr(0, kv.find('=')); const int v = atoi(kv.c_str() + kv.find('=') + 1);
            if (name == "R64") r.r64 = v; else if (name == "SPLITK") r.splitk = v; else if (name == "SKINNY") r.skinny = v;
            else if (name == "SKINNY_MAXN") r.skinny_max_n = r.skinny_max_n_few = v; else if (name == "WIDE") r.wide = v; else if (name == "R64S") r.r64s = v;
            else if (name == "PREP_REG") r.prep_reg = v; else if (name == "REGB_Q23") r.regb_q23 = v; else if (name == "MM_GROUP") r.mm_group = v;
            else if (name == "SPLITK_COMBINE") r.splitk_combine = v; else if (name == "BF16") r.prec = v ? QMM_PREC_BF16 : QMM_PREC_F16_Q8;
            else if (name == "Q8") r.prec = v ? QMM_PREC_Q8_EXACT : QMM_PREC_F16_Q8; else return 1;
        }
        PrefillGroupPlan g;
        prefill_group_plan(g, r, ws.data(), (int) ws.size(), K, N, flags);
        if (g.error) { printf("refused: %s\n", g.error); continue; }
        for (int k = 0; k < g.n; ++k) {
            const PrefillEntry & e = g.e[k];
            if (e.plan.per_matrix || e.n < 1 || e.n > 4) return 2;
            printf("%d..%d %s%s %s%s; ", e.first, e.first + e.n - 1, e.plan.label, e.plan.combine_ok ? "+combine" : "", e.prep ? "prep=" : "reuse", e.prep ? e.plan.prep_label : "");
        }
        printf("ws=%zu\n", g.ws_total);
    }
    return 0;
}
"""
# (group, its launches in issue order).  A group: CUs, the weight type id and the rows of each matrix, K, tokens, flags (2 = SwiGLU input,
# 4 = fused norm), switches off their defaults (Q8=1: QMM_PREC_Q8_EXACT).  A launch: first..last matrix, the MFMA label, then the prep it
# goes behind or "reuse" (the operand of the launch before it); last the workspace bytes of the call.
# The right-hand sides were printed by the code of the commit before prefill_group_plan existed: mul_mat_group_impl's run-cutting loop,
# its re-use test (side streams off) and mfma_mul_mat's per-matrix recursion, copied into a stand-alone program on that commit's plan
# header, never by this function: q / k / v as one launch and per matrix, mixed types with one key and with two, one type cut by key,
# keys A, B, A, rows of zero, more than 4 of a type, 9 and 8 runs, each flag, Q8-exact, other chip sizes, the switches a group meets.
GROUP_TABLE = [
    ("256 12,12,12 4096,1024,1024 4096 512 0",
     "0..2 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; ws=29362432"),
    ("256 12,12,12 4096,1024,1024 4096 512 0 MM_GROUP=0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_regb_kernel<12,8,128> reuse; 2..2 mfma_regb_kernel<12,8,128> reuse; ws=37751040"),
    ("256 12,12,12 4096,1024,1024 4096 100 0",
     "0..0 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<12,8,2> reuse; 2..2 mfma_skinny_kernel<12,8,2> reuse; ws=1049344"),
    ("256 12,12,12 4096,1024,1024 4096 9 0",
     "0..0 mfma_skinny_kernel<12,8,1> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<12,8,1> reuse; 2..2 mfma_skinny_kernel<12,8,1> reuse; ws=1049344"),
    ("256 12,12,12 4096,1024,1024 4096 129 0",
     "0..2 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; ws=17949952"),
    ("256 12,12,14 4096,1024,1024 4096 512 0",
     "0..1 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 2..2 mfma_regb_kernel<14,8,128> reuse; ws=35653888"),
    ("256 12,12,14 4096,1024,1024 4096 33 0",
     "0..0 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<12,8,2> reuse; 2..2 mfma_skinny_kernel<14,8,2> prep=prep_act_q8k_kernel<3>; ws=1049344"),
    ("256 12,12,14 4096,1024,1024 4096 33 0 SKINNY=0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_regb_kernel<12,8,128> reuse; 2..2 mfma_regb_kernel<14,8,128> reuse; ws=5374720"),
    ("256 12,12 16384,4096 4096 100 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; ws=27263744"),
    ("256 12,12 8224,96 1024 100 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; ws=6842112"),
    ("304 12,12 8224,96 1024 100 0",
     "0..0 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<12,8,2> reuse; ws=262912"),
    ("64 12,12 16384,4096 4096 100 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_regb_kernel<12,8,128> reuse; ws=7602944"),
    ("256 12,2,12 256,128,96 1024 33 0",
     "0..0 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<2,8,2> prep=prep_act_kernel<8>; 2..2 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; ws=262912"),
    ("256 12,2,12 256,128,96 1024 200 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_regb_kernel<2,8,128> prep=prep_act_kernel<8>; 2..2 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; ws=935168"),
    ("256 12,12,12 4096,0,1024 4096 512 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 2..2 mfma_regb_kernel<12,8,128> reuse; ws=37751040"),
    ("256 12,14,12 4096,0,1024 4096 512 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 2..2 mfma_regb_kernel<12,8,128> reuse; ws=37751040"),
    ("256 12,12 0,0 4096 512 0",
     "ws=0"),
    ("256 12,12,12,12,12 1024,1024,1024,1024,1024 4096 512 0",
     "0..3 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 4..4 mfma_regb_kernel<12,8,128> reuse; ws=37751040"),
    ("256 12,12,12,12,14,14 4096,1024,1024,4096,1024,1024 4096 512 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_regb_kernel<12,8,128> reuse; 2..2 mfma_regb_kernel<12,8,128> reuse; 3..3 mfma_regb_kernel<12,8,128> reuse; 4..5 mfma_regb_kernel<14,8,128> reuse; ws=37751040"),
    ("256 12,14,12,14,12,14,12,14,12 256,256,256,256,256,256,256,256,256 1024 33 0",
     "refused: too many runs in one group"),
    ("256 12,14,12,14,12,14,12,14 256,256,256,256,256,256,256,256 1024 33 0",
     "0..0 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 1..1 mfma_skinny_kernel<14,8,2> prep=prep_act_q8k_kernel<3>; 2..2 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 3..3 mfma_skinny_kernel<14,8,2> prep=prep_act_q8k_kernel<3>; 4..4 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 5..5 mfma_skinny_kernel<14,8,2> prep=prep_act_q8k_kernel<3>; 6..6 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2>; 7..7 mfma_skinny_kernel<14,8,2> prep=prep_act_q8k_kernel<3>; ws=262912"),
    ("256 12 4096 14336 512 2",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; ws=48236800"),
    ("256 14,14 4096,4096 14336 512 2",
     "0..1 mfma_regb_kernel<14,8,128> prep=prep_act_q8k_kernel<3>; ws=48236800"),
    ("256 12,12,14 4096,1024,1024 4096 512 4",
     "0..1 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2,norm>; 2..2 mfma_regb_kernel<14,8,128> reuse; ws=35653888"),
    ("256 12,14,12 256,128,96 4096 33 4",
     "0..0 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2,norm>; 1..1 mfma_skinny_kernel<14,8,2> prep=prep_act_q8k_kernel<3,norm>; 2..2 mfma_skinny_kernel<12,8,2> prep=prep_act_q8k_kernel<2,norm>; ws=1049344"),
    ("256 2,2 4096,4096 4096 512 4",
     "0..1 mfma_regb_kernel<2,8,128> prep=prep_act_kernel<8>; ws=37751040"),
    ("256 12,12,12 4096,1024,1024 4096 512 0 Q8=1",
     "0..0 mfma_q8x_kernel<12> prep=prep_act_q8x_kernel; 1..1 mfma_q8x_kernel<12> reuse; 2..2 mfma_q8x_kernel<12> reuse; ws=2130176"),
    ("256 12,2,12 4096,1024,1024 4096 512 0 Q8=1",
     "0..0 mfma_q8x_kernel<12> prep=prep_act_q8x_kernel; 1..1 mfma_regb_kernel<2,8,128> prep=prep_act_kernel<8>; 2..2 mfma_q8x_kernel<12> prep=prep_act_q8x_kernel; ws=20973824"),
    ("256 12,12,14 4096,1024,1024 4096 33 0 Q8=1",
     "0..0 mfma_q8x_kernel<12> prep=prep_act_q8x_kernel; 1..1 mfma_q8x_kernel<12> reuse; 2..2 mfma_q8x_kernel<14> reuse; ws=137728"),
    ("256 12,14 4096,1024 4096 512 4 Q8=1",
     "0..0 mfma_q8x_kernel<12> prep=prep_act_q8x_kernel; 1..1 mfma_q8x_kernel<14> reuse; ws=2130176"),
    ("304 12,12,12 4096,1024,1024 4096 512 0",
     "0..2 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; ws=41945344"),
    ("64 12,12,14 4096,1024,1024 4096 512 0",
     "0..1 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 2..2 mfma_regb_kernel<14,8,128> reuse; ws=12585216"),
    ("256 2,2,2 4096,4096,4096 4096 512 0",
     "0..0 mfma_regb_kernel<2,8,128> prep=prep_act_kernel<8>; 1..1 mfma_regb_kernel<2,8,128> reuse; 2..2 mfma_regb_kernel<2,8,128> reuse; ws=37751040"),
    ("256 12,12 14336,14336 4096 512 0",
     "0..1 mfma_r64s_q4k_kernel<2> prep=prep_act_q8k_kernel<2>; ws=4196608"),
    ("256 12,12 14336,14336 4096 512 0 R64S=0",
     "0..1 mfma_r64_q4k_kernel<8> prep=prep_act_q8k_kernel<2>; ws=4196608"),
    ("256 12,12 14336,14336 4096 512 0 WIDE=0",
     "0..1 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; ws=4196608"),
    ("256 12,13 4096,4096 4096 512 0",
     "0..0 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; 1..1 mfma_regb_kernel<13,8,128> reuse; ws=37751040"),
    ("256 14,14 4096,1024 4096 512 0 BF16=1",
     "0..0 mfma_kernel<14,64> prep=prep_act_kernel<15>; 1..1 mfma_kernel<14,64> reuse; ws=4196608"),
    ("256 12,12,12 4096,1024,1024 4096 512 0 SPLITK_COMBINE=1",
     "0..2 mfma_regb_kernel<12,8,128>+combine prep=prep_act_q8k_kernel<2>; ws=29362432"),
    ("256 11,11 4096,1024 4096 512 0 REGB_Q23=0",
     "0..0 mfma_kernel<11,64> prep=prep_act_q8k_kernel<0>; 1..1 mfma_kernel<11,64> reuse; ws=4196608"),
    ("256 14 32000 4096 512 0",
     "0..0 mfma_regb_kernel<14,8,128> prep=prep_act_q8k_kernel<3>; ws=4196608"),
    ("256 8,8,12 1024,1024,4096 4096 512 0",
     "0..1 mfma_regb_kernel<8,8,128> prep=prep_act_kernel<8>; 2..2 mfma_regb_kernel<12,8,128> prep=prep_act_q8k_kernel<2>; ws=37751040"),
]


@pytest.fixture(scope="module")
def group_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler into a program that prints the group plan of each group on its input"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("group")
    (d / "probe.cpp").write_text(GROUP_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_prefill_group_plan_keeps_every_decision(group_probe):
    assert len(GROUP_TABLE) >= 30
    got = group_probe([spec for spec, _ in GROUP_TABLE])
    assert len(got) == len(GROUP_TABLE)
    for (spec, want), line in zip(GROUP_TABLE, got):
        assert line == want, spec


def test_prefill_group_rules_live_in_the_plan_header_only():
    """how a group is cut into runs is the plan's own: no other file in csrc/ calls prefill_prep_key (comments may speak of it), and
    the context has no member through which a prefill call would talk to its callees, nor side streams"""
    csrc = ROOT / "ggml-hexagon_amd" / "csrc"
    for f in sorted(csrc.iterdir()):
        if f == PLAN_HEADER or f.suffix not in (".cpp", ".h", ".hip", ".hiph"):
            continue
        for n, line in enumerate(f.read_text().splitlines(), 1):
            code = re.sub(r"//.*$", "", line)
            assert not re.search(r"\bprefill_prep_key\b", code), f"{f.name}:{n}: {line.strip()[:120]}"
    for n, line in enumerate((csrc / "qmm_host.h").read_text().splitlines(), 1):
        code = re.sub(r"//.*$", "", line)
        assert not re.search(r"\b(prep_x2|prep_ldx2|prep_norm|ws_base|ws_used|side|side_on)\b", code), f"qmm_host.h:{n}: {line.strip()[:120]}"


# ---- the few-token launch plan (csrc/qmm_matvec_plan.h): kernel, instantiation, grid, block and LDS of the N <= 8 mat-vec paths

MV_PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_matvec_plan.h"
MV_PLAN_PROBE = r"""
#include "qmm_matvec_plan.h"
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
using namespace qmm;
static std::vector<int64_t> csv(const std::string & s) {
    std::vector<int64_t> v; std::istringstream in(s); std::string x;
    while (std::getline(in, x, ',')) v.push_back(atoll(x.c_str()));
    return v;
}
// the plan of one spec as a line.  group: cus types M.. K N extras [NAME=VAL ...]; step (a chain step launched alone): the same
// without N; moe: cus form type K M pairs
static std::string plan_line(const std::string & spec) {
    std::istringstream in(spec);
    std::string what, ts, ms, exs, kv;
    char b[256], t[96];
    std::string out;
    in >> what;
    if (what == "moe") {
        int cus, form, type, K, M, P;
        in >> cus >> form >> type >> K >> M >> P;
        if (!moe_runs_as_matvec(1, P)) return "not as mat-vecs";
        const MoeMatvecPlan p = moe_matvec_plan(cus, form, type, K, M, P);
        p.text(t, sizeof(t));
        snprintf(b, sizeof(b), "%s grid=%u,%u,%u block=%u lds=%zu", t, p.grid[0], p.grid[1], p.grid[2], p.block, p.lds);
        return b;
    }
    MatvecRules r = { 256, 1, 2, 1, QMM_ACT_REF };                  // qmm_ctx's defaults
    if (what == "sweep") {
        // sweep types: whatever a fit estimate accepts, the launch it stands for asks for no more than MV_LDS_LAUNCH: every type, 1 .. 8
        // tokens, K in multiples of the type's block (planar rows: of 256) up to 32768, as mv_same_bytes walks them
        in >> ts;
        long long checked = 0;
        size_t worst = 0;
        const int re[1] = { 8 };
        auto over = [&](int kind, int type, int K, int n, bool norm, int swiglu, const char * fit) {
            const MatvecLaunch l = matvec_launch(r, kind, type, nullptr, re, 1, K, 0, n, norm, swiglu, nullptr);
            ++checked;
            if (l.lds > worst) worst = l.lds;
            if (l.lds <= MV_LDS_LAUNCH) return false;
            snprintf(b, sizeof(b), "sweep violation: %s accepts kind %d type %d n=%d K=%d, the launch needs %zu B", fit, kind, type, n, K, l.lds);
            return true;
        };
        for (int64_t type : csv(ts)) {
            const int ty = (int) type, step = type_planar(ty) ? 256 : type_blck(ty);
            for (int K = step; K <= 32768; K += step) for (int n = 1; n <= QMM_MATVEC_MAX_N; ++n) {
                if (mv_fits_plain(n, K) && over(MV_PER_TYPE, ty, K, n, false, 0, "mv_fits_plain")) return b;
                if (mv_fits_norm(n, K) && over(MV_PER_TYPE, ty, K, n, true, 0, "mv_fits_norm")) return b;
                if (mv_fits_swiglu(n, K, false) && over(MV_PER_TYPE, ty, K, n, false, 1, "mv_fits_swiglu")) return b;
                if (mv_fits_swiglu(n, K, true) && over(MV_PER_TYPE, ty, K, n, true, 1, "mv_fits_swiglu with the norm")) return b;
                if (K % 256) continue;
                if (mv_fits_mixed(n, K) && over(MV_MIXED, ty, K, n, false, 0, "mv_fits_mixed")) return b;
                if (mv_fits_mixed(n, K) && mv_fits_norm(n, K) && over(MV_MIXED, ty, K, n, true, 0, "mv_fits_mixed with the norm")) return b;
                if (mv_fits_mixed_q80(n, K) && n <= 4 && over(MV_MIXED_Q80, ty, K, n, false, 0, "mv_fits_mixed_q80")) return b;
            }
        }
        snprintf(b, sizeof(b), "sweep ok: %lld launches, the largest %zu B", checked, worst);
        return b;
    }
    int64_t K, N = 1;
    in >> r.cus >> ts >> ms >> K;
    if (what == "group") in >> N;
    in >> exs;
    while (in >> kv) {
        const std::string name = kv.substr(0, kv.find('=')); const int v = atoi(kv.c_str() + kv.find('=') + 1);
        if (name == "MV_BPC") r.mv_bpc = v; else if (name == "MV_KMIX") r.mv_kmix = v; else if (name == "MV_ONEPASS") r.mv_onepass = v;
        else if (name == "ACT_MODE") r.act_mode = v ? QMM_ACT_X86 : QMM_ACT_REF; else return "bad spec";
    }
    const std::vector<int64_t> types = csv(ts), M = csv(ms);
    const int nw = (int) types.size();
    std::vector<qmm_weight> ws(nw);
    for (int i = 0; i < nw; ++i) { ws[i] = qmm_weight{}; ws[i].type = (int) types[i]; ws[i].M = M[i]; }
    // extras: "-" none, else letters: n norm, b norm weight misaligned, s<1|2|3> swiglu, r<i> residual of matrix i, e nothing set
    qmm_mv_extra ex = {};
    for (size_t i = 0; i < exs.size(); ++i) {
        if (exs[i] == 'n') ex.norm_w = (const float *) (uintptr_t) 4096;
        if (exs[i] == 'b') ex.norm_w = (const float *) (uintptr_t) 4100;
        if (exs[i] == 's') ex.swiglu = exs[++i] - '0';
        if (exs[i] == 'r') ex.residual[exs[++i] - '0'] = (const float *) (uintptr_t) 8192;
    }
    const qmm_mv_extra * exp = exs == "-" ? nullptr : &ex;
    auto add = [&](const MatvecLaunch & l) {
        l.text(t, sizeof(t));
        if (!out.empty()) out += "; ";
        if (l.error) { snprintf(b, sizeof(b), "refused %d: %s", l.error, t); out += b; return false; }
        std::string m;
        for (int k = 0; k < l.n; ++k) { snprintf(b, sizeof(b), "%s%d:%d", k ? "," : "", l.idx[k], l.row_end[k]); m += b; }
        snprintf(b, sizeof(b), "%s m=%s n0=%d grid=%d block=%d lds=%zu arg=%d", t, m.c_str(), l.n0, l.blocks, l.waves * 64, l.lds, l.act_arg);
        out += b;
        return true;
    };
    if (what == "step") {
        int te[MV_MAX_GROUP] = {}, re[MV_MAX_GROUP] = {}, rows = 0;
        bool res = false;
        for (int i = 0; i < nw; ++i) { te[i] = ws[i].type; re[i] = rows += (int) ws[i].M; res = res || ex.residual[i]; }
        add(matvec_launch(r, mv_kind_of(te, nw), te[0], nullptr, re, nw, (int) K, 0, 1, ex.norm_w != nullptr, ex.swiglu, res ? ex.residual : nullptr));
        return out;
    }
    if (exp) {
        char msg[160];
        const int rc = matvec_extras_check(ws.data(), nw, K, N, exp, msg, sizeof(msg));
        if (rc) { snprintf(b, sizeof(b), "refused %d: %s", rc, msg); return b; }
    }
    for (int first = 0; first < nw;) {
        const MatvecPlan p = matvec_group_plan(r, ws.data(), nw, K, N, exp, first);
        for (int k = 0; k < p.n; ++k) if (!add(p.launch[k])) return out;
        first = p.next;
    }
    return out.empty() ? "nothing" : out;
}
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) printf("%s\n", plan_line(spec).c_str());
    return 0;
}
"""
# (spec, what the launch code did with it before the plan existed).  "group": CUs, the weight type ids and the rows of the call's matrices, K,
# tokens, the extras ("-": a plain call; n = norm, b = a misaligned norm weight, s1 / s2 = swiglu, r<i> = residual of matrix i, e = extras
# with nothing set), switches off their defaults.  "step": a chain step launched on its own (one token).  "moe": CUs, form (0 = one expert
# tensor, 1 = a pair, 2 = the pair with the SwiGLU folded), type, K, rows, (token, slot) pairs.  A launch: its trace label, m = matrix:cumulative
# rows, first token, grid, block, LDS bytes, the act_mode argument.
# The right-hand sides were printed by the decision code of the commit before this header (mul_mat_group_impl, launch_matvec_n, launch_kmix_n,
# chain_step_plain, launch_matvec_id, launch_matvec_id_swiglu, moe_mul_mat_id) copied into a stand-alone program, never by the header: every
# distinct token-generation group of the five BASELINE workloads at one token, the forms the plugin folds a layer into, the token counts
# around the kernels' bounds, the mixed-type and mixed-format groups at their LDS limits, sub-batches, every refusal, other chip sizes,
# each mat-vec switch off its default, and MoE around MOE_MATVEC_MAX_PAIRS.
MV_PLAN_TABLE = [
    ("group 256 2,2,2 4096,4096,4096 4096 1 -",
     "matvec_kernel<2,1,false> m=0:4096,1:8192,2:12288 n0=0 grid=256 block=1024 lds=4608 arg=0"),
    ("group 256 2 4096 4096 1 -",
     "matvec_kernel<2,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=4608 arg=0"),
    ("group 256 2,2 11008,11008 4096 1 -",
     "matvec_kernel<2,1,false> m=0:11008,1:22016 n0=0 grid=256 block=1024 lds=4608 arg=0"),
    ("group 256 2 4096 11008 1 -",
     "matvec_kernel<2,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=12384 arg=0"),
    ("group 256 14 32000 4096 1 -",
     "matvec_kernel<14,1,false> m=0:32000 n0=0 grid=256 block=1024 lds=4672 arg=0"),
    ("group 256 12,12,14 4096,1024,1024 4096 1 -",
     "matvec_kmix_kernel<1,false> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=4672 arg=0"),
    ("group 256 12,12,12 4096,1024,1024 4096 1 -",
     "matvec_kernel<12,1,false> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 12 4096 4096 1 -",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 12,12 14336,14336 4096 1 -",
     "matvec_kernel<12,1,false> m=0:14336,1:28672 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 14 4096 14336 1 -",
     "matvec_kernel<14,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=16352 arg=0"),
    ("group 256 12 4096 14336 1 -",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=15456 arg=0"),
    ("group 256 14 128256 4096 1 -",
     "matvec_kernel<14,1,false> m=0:128256 n0=0 grid=256 block=1024 lds=4672 arg=0"),
    ("group 256 12,12,14 8192,1024,1024 8192 1 -",
     "matvec_kmix_kernel<1,false> m=0:8192,1:9216,2:10240 n0=0 grid=256 block=1024 lds=9344 arg=0"),
    ("group 256 12,12,13 8192,1024,1024 8192 1 -",
     "matvec_kmix_kernel<1,false> m=0:8192,1:9216,2:10240 n0=0 grid=256 block=1024 lds=9344 arg=0"),
    ("group 256 12 8192 8192 1 -",
     "matvec_kernel<12,1,false> m=0:8192 n0=0 grid=256 block=1024 lds=8832 arg=0"),
    ("group 256 12,12 28672,28672 8192 1 -",
     "matvec_kernel<12,1,false> m=0:28672,1:57344 n0=0 grid=256 block=1024 lds=8832 arg=0"),
    ("group 256 14 8192 28672 1 -",
     "matvec_kernel<14,1,false> m=0:8192 n0=0 grid=256 block=1024 lds=32704 arg=0"),
    ("group 256 12 8192 28672 1 -",
     "matvec_kernel<12,1,false> m=0:8192 n0=0 grid=256 block=1024 lds=30912 arg=0"),
    ("group 256 14 128256 8192 1 -",
     "matvec_kernel<14,1,false> m=0:128256 n0=0 grid=256 block=1024 lds=9344 arg=0"),
    ("group 256 12,8,8 4096,1024,1024 4096 1 -",
     "matvec_kmix_kernel<1,false,q8_0> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=9280 arg=0"),
    ("group 256 13 4096 4096 1 -",
     "matvec_kernel<13,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("moe 256 1 12 4096 14336 2",
     "matvec_id_kernel<12> grid=2,128,2 block=512 lds=4416"),
    ("moe 256 0 14 14336 4096 2",
     "matvec_id_kernel<14> grid=2,256,1 block=512 lds=16352"),
    ("moe 256 0 12 14336 4096 2",
     "matvec_id_kernel<12> grid=2,256,1 block=512 lds=15456"),
    ("group 256 12,12,12 4096,4096,4096 4096 1 -",
     "matvec_kernel<12,1,false> m=0:4096,1:8192,2:12288 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 12,12 11008,11008 4096 1 -",
     "matvec_kernel<12,1,false> m=0:11008,1:22016 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 12 4096 11008 1 -",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=11872 arg=0"),
    ("group 256 12 32000 4096 1 -",
     "matvec_kernel<12,1,false> m=0:32000 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 12,12,14 4096,1024,1024 4096 1 n",
     "matvec_kmix_kernel<1,true> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=21056 arg=0"),
    ("group 256 12,12 14336,14336 4096 1 ns1",
     "matvec_kernel<12,1,true> m=0:14336,1:28672 n0=0 grid=256 block=1024 lds=20800 arg=0"),
    ("group 256 12,12 14336,14336 4096 1 s2",
     "matvec_kernel<12,1,true> m=0:14336,1:28672 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 14 4096 14336 1 r0",
     "matvec_kernel<14,1,true> m=0:4096 n0=0 grid=256 block=1024 lds=16352 arg=0"),
    ("group 256 12,12,14 4096,1024,1024 4096 4 -",
     "matvec_kmix_kernel<4,false> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=18688 arg=0"),
    ("group 256 12,12,14 4096,1024,1024 4096 5 -",
     "matvec_kmix_kernel<5,false> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=23360 arg=0"),
    ("group 256 12,12,14 4096,1024,1024 4096 8 n",
     "refused -5: qmm_mul_mat_group_ex: 8 rows of 4096 do not fit LDS with the norm"),
    ("group 256 12,8,8 4096,1024,1024 4096 4 -",
     "matvec_kmix_kernel<4,false,q8_0> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=37120 arg=0"),
    ("group 256 12,8,8 4096,1024,1024 4096 5 -",
     "matvec_kernel<12,5,false> m=0:4096 n0=0 grid=256 block=1024 lds=22080 arg=0; matvec_kernel<8,5,false> m=1:1024,2:2048 n0=0 grid=256 block=512 lds=23040 arg=0"),
    ("group 256 12,8,8 4096,1024,1024 14336 3 -",
     "matvec_kmix_kernel<3,false,q8_0> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=97440 arg=0"),
    ("group 256 12,8,8 4096,1024,1024 14336 4 -",
     "matvec_kernel<12,4,false> m=0:4096 n0=0 grid=256 block=1024 lds=61824 arg=0; matvec_kernel<8,4,false> m=1:1024,2:2048 n0=0 grid=256 block=512 lds=64512 arg=0"),
    ("group 256 12,8,8 4096,1024,1024 4096 1 - MV_KMIX=1",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=4416 arg=0; matvec_kernel<8,1,false> m=1:1024,2:2048 n0=0 grid=256 block=512 lds=4608 arg=0"),
    ("group 256 12,8,8 4096,1024,1024 4096 1 n",
     "matvec_kernel<12,1,true> m=0:4096 n0=0 grid=256 block=1024 lds=20800 arg=0; matvec_kernel<8,1,true> m=1:1024,2:2048 n0=0 grid=256 block=512 lds=20992 arg=0"),
    ("group 256 12,12,14 4096,1024,1024 4096 1 - MV_KMIX=0",
     "matvec_kernel<12,1,false> m=0:4096,1:5120 n0=0 grid=256 block=1024 lds=4416 arg=0; matvec_kernel<14,1,false> m=2:1024 n0=0 grid=256 block=256 lds=4672 arg=0"),
    ("group 256 12 4096 28672 8 -",
     "matvec_kernel<12,4,false> m=0:4096 n0=0 grid=256 block=1024 lds=123648 arg=0; matvec_kernel<12,4,false> m=0:4096 n0=4 grid=256 block=1024 lds=123648 arg=0"),
    ("group 256 12 4096 14336 8 -",
     "matvec_kernel<12,8,false> m=0:4096 n0=0 grid=256 block=1024 lds=123648 arg=0"),
    ("group 256 2,2 11008,11008 4096 5 -",
     "matvec_kernel<2,5,false> m=0:11008,1:22016 n0=0 grid=256 block=1024 lds=23040 arg=0"),
    ("group 256 12,12 14336,0 4096 4 -",
     "matvec_kernel<12,4,false> m=0:14336 n0=0 grid=256 block=1024 lds=17664 arg=0"),
    ("group 256 12,0,14 4096,0,1024 4096 1 -",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=4416 arg=0; matvec_kernel<14,1,false> m=2:1024 n0=0 grid=256 block=256 lds=4672 arg=0"),
    ("group 256 12,12 14336,14336 8192 4 n",
     "refused -5: qmm_mul_mat_group_ex: 4 rows of 8192 do not fit LDS with the norm"),
    ("group 256 12,12 14336,14336 14336 8 s1",
     "matvec_kernel<12,8,true> m=0:14336,1:28672 n0=0 grid=256 block=1024 lds=123648 arg=0"),
    ("group 256 12,12 14336,14336 4096 1 s1r0",
     "refused -5: qmm_mul_mat_group_ex: swiglu wants two matrices of one type and shape, no residuals, all tokens in one launch"),
    ("group 256 12,14 14336,14336 4096 1 s1",
     "refused -5: qmm_mul_mat_group_ex: swiglu wants two matrices of one type and shape, no residuals, all tokens in one launch"),
    ("group 256 12,12 14336,14336 4096 1 b",
     "refused -1: qmm_mul_mat_group_ex: norm weight must be 16-byte aligned, eps >= 0"),
    ("group 256 12,12 4096,4096 4096 9 n",
     "refused -5: qmm_mul_mat_group_ex: batches of <= 8 tokens, <= 4 matrices"),
    ("group 256 12 4096 4096 1 e",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 3 4096 163840 1 -",
     "refused -5: matvec: 1 tokens x K=163840 needs 204800 B of LDS"),
    ("group 256 12,12,14 4096,1024,1024 4096 1 n MV_ONEPASS=0",
     "matvec_kmix_kernel<1,true> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=21056 arg=256"),
    ("group 256 12 4096 4096 1 - MV_BPC=2",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    ("group 256 12 32000 4096 1 - MV_BPC=2",
     "matvec_kernel<12,1,false> m=0:32000 n0=0 grid=512 block=1024 lds=4416 arg=0"),
    ("group 256 12 4096 4096 2 - ACT_MODE=1",
     "matvec_kernel<12,2,false> m=0:4096 n0=0 grid=256 block=1024 lds=8832 arg=1"),
    ("group 64 12,12,14 4096,1024,1024 4096 1 -",
     "matvec_kmix_kernel<1,false> m=0:4096,1:5120,2:6144 n0=0 grid=64 block=1024 lds=4672 arg=0"),
    ("group 64 12 4096 4096 1 -",
     "matvec_kernel<12,1,false> m=0:4096 n0=0 grid=64 block=1024 lds=4416 arg=0"),
    ("group 304 12,12 14336,14336 4096 1 -",
     "matvec_kernel<12,1,false> m=0:14336,1:28672 n0=0 grid=304 block=1024 lds=4416 arg=0"),
    ("group 304 14 1024 4096 1 -",
     "matvec_kernel<14,1,false> m=0:1024 n0=0 grid=256 block=256 lds=4672 arg=0"),
    ("group 256 12,12,12,12,12 1024,1024,1024,1024,1024 4096 1 -",
     "matvec_kernel<12,1,false> m=0:1024,1:2048,2:3072,3:4096 n0=0 grid=256 block=1024 lds=4416 arg=0; matvec_kernel<12,1,false> m=4:1024 n0=0 grid=256 block=256 lds=4416 arg=0"),
    ("step 256 12,12,14 4096,1024,1024 4096 n",
     "matvec_kmix_kernel<1,true> m=0:4096,1:5120,2:6144 n0=0 grid=256 block=1024 lds=21056 arg=0"),
    ("step 256 12,12 14336,14336 4096 s1",
     "matvec_kernel<12,1,true> m=0:14336,1:28672 n0=0 grid=256 block=1024 lds=4416 arg=0"),
    # (pins what the parent did, not what is right: a chain step that holds Q4_0 and Q8_0 matrices, both Q8_0 activations, and goes out alone
    # is sent to matvec_kmix_kernel, which has no Q4_0 dot and takes Q8_0 rows only as Q80.  Chains are opt-in and such a step needs a chain
    # of one; the fix is a behaviour change and not part of this refactor)
    ("step 256 2,8 4096,1024 4096 -",
     "matvec_kmix_kernel<1,false> m=0:4096,1:5120 n0=0 grid=256 block=1024 lds=4672 arg=0"),
    ("step 304 14 4096 14336 r0",
     "matvec_kernel<14,1,true> m=0:4096 n0=0 grid=256 block=1024 lds=16352 arg=0"),
    ("moe 256 0 12 4096 14336 16",
     "matvec_id_kernel<12> grid=16,32,1 block=512 lds=4416"),
    ("moe 256 0 12 4096 14336 17",
     "not as mat-vecs"),
    ("moe 256 1 12 4096 14336 16",
     "matvec_id_kernel<12> grid=16,16,2 block=512 lds=4416"),
    ("moe 256 1 12 4096 14336 17",
     "not as mat-vecs"),
    ("moe 256 2 12 4096 14336 2",
     "matvec_id_swiglu_kernel<12> grid=2,256,1 block=512 lds=4416"),
    ("moe 256 2 12 4096 14336 16",
     "matvec_id_swiglu_kernel<12> grid=16,32,1 block=512 lds=4416"),
    ("moe 256 2 12 4096 14336 17",
     "not as mat-vecs"),
    ("moe 64 1 8 4096 512 2",
     "matvec_id_kernel<8> grid=2,32,2 block=512 lds=4608"),
    ("moe 304 2 14 14336 7 16",
     "matvec_id_swiglu_kernel<14> grid=16,1,1 block=512 lds=16352"),
]


@pytest.fixture(scope="module")
def mv_plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each spec on its input"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("mvplan")
    (d / "probe.cpp").write_text(MV_PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{MV_PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_matvec_plan_keeps_every_decision(mv_plan_probe):
    assert len(MV_PLAN_TABLE) >= 40
    got = mv_plan_probe([spec for spec, _ in MV_PLAN_TABLE])
    assert len(got) == len(MV_PLAN_TABLE)
    for (spec, want), line in zip(MV_PLAN_TABLE, got):
        assert line == want, spec


def test_matvec_rules_live_in_the_plan_header_only():
    """the launchers the plan replaced are gone, and no other file in csrc/ spells an LDS budget or a fit formula (comments may speak of them)"""
    for f in sorted((ROOT / "ggml-hexagon_amd" / "csrc").iterdir()):
        if f == MV_PLAN_HEADER or f.suffix not in (".cpp", ".h", ".hip", ".hiph"):
            continue
        for n, line in enumerate(f.read_text().splitlines(), 1):
            code = re.sub(r"//.*$", "", line)
            where = f"{f.name}:{n}: {line.strip()[:120]}"
            assert not re.search(r"\b(launch_matvec_n|launch_kmix_n|launch_kmix|launch_matvec|launch_matvec_id_swiglu|matvec_any|group_has_extras|kmix_lds_bytes|type_ok|blck|tsize)\b", code), where
            assert not re.search(r"\b1(5|6)0\s*(\*\s*1024|<<\s*10)\b|\b1(536|638)00\b", code), where
            assert not re.search(r"\*\s*(\w+(\.|->))?k\s*\*\s*(5\s*/\s*4|11\s*/\s*8|21\s*/\s*8)", code, re.I), where
            assert not re.search(r"MOE_MATVEC_MAX_PAIRS *=", code), where


# ---- the attention launch plan (csrc/qmm_attn_plan.h): kernel, instantiation, grid, block, LDS and the pieces of a cut cache

ATTN_PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_attn_plan.h"
ATTN_SECTION = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_attn.hiph"
ATTN_PLAN_PROBE = r"""
#include "qmm_attn_plan.h"
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {          // D Dv n_kv N H fresh [SHORT=0] [SPLIT=0]  |  prefill D n_kv N H
        std::istringstream in(spec);
        std::string first, kv;
        in >> first;
        AttnPlan p;
        if (first == "prefill") {
            int D, n_kv, N, H;
            in >> D >> n_kv >> N >> H;
            p = attn_prefill_plan(D, n_kv, N, H);
        } else {
            AttnRules r = { true, true };
            int Dv, n_kv, N, H, fresh;
            in >> Dv >> n_kv >> N >> H >> fresh;
            while (in >> kv) { if (kv == "SHORT=0") r.short_on = false; else if (kv == "SPLIT=0") r.split_on = false; else return 1; }
            p = attn_decode_plan(r, atoi(first.c_str()), Dv, n_kv, N, H, fresh != 0);
        }
        printf("%s%s%s grid=%u,%u,%u block=%u lds=%zu attr=%d S=%d chunk=%d ws=%zu\n", p.label, p.label2[0] ? ";" : "", p.label2, p.grid[0], p.grid[1], p.grid[2],
               p.block, p.lds, (int) p.lds_attr, p.S, p.chunk, p.ws_bytes);
    }
    return 0;
}
"""
# (shape, what the launchers did with it before the plan existed).  A shape: D, Dv, n_kv, tokens, heads, fresh (1 = qmm_attn_decode_rope: the
# batch's own K / V rows come with the launch) and the switches off their defaults; or "prefill" D, n_kv, tokens, heads.  The right-hand sides
# were printed by the launch code of the commit before this header (qmm_attn_decode, qmm_attn_decode_rope, qmm_attn_prefill of qmm_ops.hip)
# copied into a stand-alone program, never by the header; the labels name the instantiation that code's ladders picked.  attr: the launcher
# raised the kernel's LDS limit first.  Every width of the short kernel at both of its ends, the first and the longest cache the split takes,
# ragged pieces, D = 256, Dv > 128, fresh rows at each width and past them, one fresh launch past 64 KiB, each switch where it changes the answer.
ATTN_PLAN_TABLE = [
    ("64 64 8 1 8 0",
     "attn_decode_short_kernel<64,false,256> grid=8,1,1 block=1024 lds=64 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 256 2 8 0",
     "attn_decode_short_kernel<64,false,256> grid=8,2,1 block=1024 lds=2048 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 264 3 8 0",
     "attn_decode_short_kernel<64,false,512> grid=8,3,1 block=1024 lds=2112 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 512 1 8 0",
     "attn_decode_short_kernel<64,false,512> grid=8,1,1 block=1024 lds=4096 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 520 2 8 0",
     "attn_decode_short_kernel<64,false,1024> grid=8,2,1 block=1024 lds=4160 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 1016 3 8 0",
     "attn_decode_short_kernel<64,false,1024> grid=8,3,1 block=1024 lds=8128 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 1024 1 8 0",
     "attn_decode_split_kernel<64>;attn_combine_kernel grid=8,1,4 block=1024 lds=1024 attr=0 S=4 chunk=256 ws=8448"),
    ("64 64 1032 2 8 0",
     "attn_decode_split_kernel<64>;attn_combine_kernel grid=8,2,4 block=1024 lds=1056 attr=0 S=4 chunk=264 ws=16896"),
    ("64 64 4096 3 8 0",
     "attn_decode_split_kernel<64>;attn_combine_kernel grid=8,3,16 block=1024 lds=1024 attr=0 S=16 chunk=256 ws=101376"),
    ("64 64 4160 1 8 0",
     "attn_decode_split_kernel<64>;attn_combine_kernel grid=8,1,16 block=1024 lds=1056 attr=0 S=16 chunk=264 ws=33792"),
    ("64 64 16384 2 8 0",
     "attn_decode_split_kernel<64>;attn_combine_kernel grid=8,2,16 block=1024 lds=4096 attr=0 S=16 chunk=1024 ws=67584"),
    ("128 128 8 1 32 0",
     "attn_decode_short_kernel<128,false,256> grid=32,1,1 block=1024 lds=64 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 256 2 32 0",
     "attn_decode_short_kernel<128,false,256> grid=32,2,1 block=1024 lds=2048 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 264 3 32 0",
     "attn_decode_short_kernel<128,false,512> grid=32,3,1 block=1024 lds=2112 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 512 1 32 0",
     "attn_decode_short_kernel<128,false,512> grid=32,1,1 block=1024 lds=4096 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 520 2 32 0",
     "attn_decode_short_kernel<128,false,1024> grid=32,2,1 block=1024 lds=4160 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 1016 3 32 0",
     "attn_decode_short_kernel<128,false,1024> grid=32,3,1 block=1024 lds=8128 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 1024 1 32 0",
     "attn_decode_split_kernel<128>;attn_combine_kernel grid=32,1,4 block=1024 lds=1024 attr=0 S=4 chunk=256 ws=66560"),
    ("128 128 1032 2 32 0",
     "attn_decode_split_kernel<128>;attn_combine_kernel grid=32,2,4 block=1024 lds=1056 attr=0 S=4 chunk=264 ws=133120"),
    ("128 128 4096 3 32 0",
     "attn_decode_split_kernel<128>;attn_combine_kernel grid=32,3,16 block=1024 lds=1024 attr=0 S=16 chunk=256 ws=798720"),
    ("128 128 4160 1 32 0",
     "attn_decode_split_kernel<128>;attn_combine_kernel grid=32,1,16 block=1024 lds=1056 attr=0 S=16 chunk=264 ws=266240"),
    ("128 128 16384 2 32 0",
     "attn_decode_split_kernel<128>;attn_combine_kernel grid=32,2,16 block=1024 lds=4096 attr=0 S=16 chunk=1024 ws=532480"),
    ("256 256 512 1 8 0",
     "attn_decode_kernel<256,false> grid=8,1,1 block=1024 lds=2048 attr=0 S=0 chunk=0 ws=0"),
    ("256 256 520 3 8 0",
     "attn_decode_kernel<256,false> grid=8,3,1 block=1024 lds=2080 attr=0 S=0 chunk=0 ws=0"),
    ("256 256 4096 1 32 0",
     "attn_decode_kernel<256,false> grid=32,1,1 block=1024 lds=16384 attr=0 S=0 chunk=0 ws=0"),
    ("64 192 264 2 8 0",
     "attn_decode_kernel<64,false> grid=8,2,1 block=1024 lds=1056 attr=0 S=0 chunk=0 ws=0"),
    ("128 192 4160 2 8 0",
     "attn_decode_split_kernel<128>;attn_combine_kernel grid=8,2,16 block=1024 lds=1056 attr=0 S=16 chunk=264 ws=198656"),
    ("128 128 256 1 8 1",
     "attn_decode_short_kernel<128,true,256> grid=8,1,1 block=1024 lds=3072 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 320 1 8 1",
     "attn_decode_short_kernel<128,true,512> grid=8,1,1 block=1024 lds=3584 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 512 2 8 1",
     "attn_decode_short_kernel<64,true,512> grid=8,2,1 block=1024 lds=4864 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 544 2 8 1",
     "attn_decode_short_kernel<128,true,1024> grid=8,2,1 block=1024 lds=5888 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 704 3 8 1",
     "attn_decode_short_kernel<128,true,1024> grid=8,3,1 block=1024 lds=7680 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 1024 1 32 1",
     "attn_decode_short_kernel<64,true,1024> grid=32,1,1 block=1024 lds=8704 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 1120 1 8 1",
     "attn_decode_kernel<128,true> grid=8,1,1 block=1024 lds=5504 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 320 8 8 1",
     "attn_decode_short_kernel<128,true,512> grid=8,8,1 block=1024 lds=7168 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 16384 1 32 1",
     "attn_decode_kernel<128,true> grid=32,1,1 block=1024 lds=66560 attr=1 S=0 chunk=0 ws=0"),
    ("64 192 256 2 8 1",
     "attn_decode_kernel<64,true> grid=8,2,1 block=1024 lds=2304 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 1024 1 8 0 SPLIT=0",
     "attn_decode_short_kernel<128,false,1024> grid=8,1,1 block=1024 lds=8192 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 4096 1 8 0 SPLIT=0",
     "attn_decode_kernel<128,false> grid=8,1,1 block=1024 lds=16384 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 256 1 8 0 SHORT=0",
     "attn_decode_kernel<128,false> grid=8,1,1 block=1024 lds=1024 attr=0 S=0 chunk=0 ws=0"),
    ("128 128 256 1 8 1 SHORT=0",
     "attn_decode_kernel<128,true> grid=8,1,1 block=1024 lds=2048 attr=0 S=0 chunk=0 ws=0"),
    ("64 64 1024 2 8 0 SHORT=0 SPLIT=0",
     "attn_decode_kernel<64,false> grid=8,2,1 block=1024 lds=4096 attr=0 S=0 chunk=0 ws=0"),
    ("prefill 64 32 33 8",
     "attn_prefill_kernel<64> grid=1,8,1 block=256 lds=27648 attr=0 S=0 chunk=0 ws=0"),
    ("prefill 128 480 200 8",
     "attn_prefill_kernel<128> grid=4,8,1 block=256 lds=142336 attr=1 S=0 chunk=0 ws=0"),
    ("prefill 128 512 512 32",
     "attn_prefill_kernel<128> grid=8,32,1 block=256 lds=150528 attr=1 S=0 chunk=0 ws=0"),
    ("prefill 128 2080 130 8",
     "attn_prefill_kernel<128> grid=3,8,1 block=256 lds=150528 attr=1 S=0 chunk=0 ws=0"),
    ("prefill 64 512 33 8",
     "attn_prefill_kernel<64> grid=1,8,1 block=256 lds=150528 attr=1 S=0 chunk=0 ws=0"),
    ("prefill 64 2080 512 32",
     "attn_prefill_kernel<64> grid=8,32,1 block=256 lds=150528 attr=1 S=0 chunk=0 ws=0"),
    ("prefill 128 96 70 8",
     "attn_prefill_kernel<128> grid=2,8,1 block=256 lds=44032 attr=0 S=0 chunk=0 ws=0"),
]


@pytest.fixture(scope="module")
def attn_plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each shape on its input"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("attnplan")
    (d / "probe.cpp").write_text(ATTN_PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{ATTN_PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_attn_plan_keeps_every_decision(attn_plan_probe):
    assert len(ATTN_PLAN_TABLE) >= 30
    got = attn_plan_probe([spec for spec, _ in ATTN_PLAN_TABLE])
    assert len(got) == len(ATTN_PLAN_TABLE)
    for (spec, want), line in zip(ATTN_PLAN_TABLE, got):
        assert line == want, spec


def test_attn_rules_live_in_one_place():
    """the plan functions and the shape predicate are defined in the plan header only; the two switches are read in one function of the
    attention section; no other file launches an attention kernel; the development harness asks the plan (comments may speak of all this)"""
    def code_of(f):
        return [re.sub(r"//.*$", "", line) for line in f.read_text().splitlines()]
    defines = re.compile(r"\b(AttnPlan|bool)\s+(attn_decode_plan|attn_prefill_plan|attn_shape_ok)\s*\(")
    assert sorted(m.group(2) for line in code_of(ATTN_PLAN_HEADER) for m in defines.finditer(line)) == ["attn_decode_plan", "attn_prefill_plan", "attn_shape_ok"]
    for f in sorted((ROOT / "ggml-hexagon_amd" / "csrc").iterdir()):
        if f.suffix not in (".cpp", ".h", ".hip", ".hiph"):
            continue
        code = code_of(f)
        inside = None                                                        # the function a line belongs to: the last line that opened one at column 0
        for n, line in enumerate(code, 1):
            where = f"{f.name}:{n}: {line.strip()[:120]}"
            if re.match(r"^\w.*\)\s*\{", line):
                inside = line
            if f != ATTN_PLAN_HEADER:
                assert not defines.search(line), where
            if f != SWITCH_HEADER and re.search(r"\bSW_ATTN_(SHORT|SPLIT)\b", line):
                assert f == ATTN_SECTION and inside is not None and re.search(r"\battn_rules\s*\(\)", inside), where
            if f != ATTN_SECTION:
                assert not re.search(r"hipLaunchKernelGGL\s*\(\s*\(*\s*attn_", line), where
    dev = (ROOT / "profiles" / "tools" / "attn_dev.hip")
    for n, line in enumerate(code_of(dev), 1):
        assert not re.search(r"n_kv\s*<=", line), f"{dev.name}:{n}: {line.strip()[:120]}"
    assert any("attn_decode_plan" in line for line in code_of(dev))


# ---- the glue launch plan (csrc/qmm_glue_plan.h): for the operands of an entry point the kernel, its instantiation, grid, block, LDS, label, refusal

GLUE_PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_glue_plan.h"
GLUE_UNIT = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_ops.hip"
GLUE_PLAN_PROBE = r"""
#include "qmm_glue_plan.h"
// one operand spec per line:  ENTRY [n_used=N] [pi<i>=INT] [pf<i>=FLOAT] NAME=TYPE:ne0[,ne1[,ne2[,ne3]]][/nb0,nb1,nb2,nb3][@ADDRESS] ...
// TYPE f32 | f16 | i32 | t<ggml type id>; strides default to contiguous; the data pointer to a 1 MiB slot of its own; pi / pf set
// op_params of the tensor named d (qd for rope_store)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
struct Spec {
    std::string entry;
    std::map<std::string, qmm_tensor> t;
    long n_used = 2;
    const qmm_tensor * get(const char * name) const { auto it = t.find(name); return it == t.end() ? nullptr : &it->second; }
};
static bool parse_spec(const std::string & line, Spec & s) {
    std::istringstream in(line);
    std::string tok;
    if (!(in >> s.entry)) return false;
    int slot = 0, pi[16] = {0};
    bool pset[16] = {false};
    while (in >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) return false;
        const std::string name = tok.substr(0, eq), val = tok.substr(eq + 1);
        if (name == "n_used") { s.n_used = atol(val.c_str()); continue; }
        if (name.size() >= 3 && name[0] == 'p' && (name[1] == 'i' || name[1] == 'f') && isdigit(name[2])) {
            const int i = atoi(name.c_str() + 2);
            if (name[1] == 'i') pi[i] = atoi(val.c_str());
            else { const float f = (float) atof(val.c_str()); memcpy(&pi[i], &f, 4); }
            pset[i] = true;
            continue;
        }
        qmm_tensor q;
        memset(&q, 0, sizeof(q));
        const size_t colon = val.find(':');
        if (colon == std::string::npos) return false;
        const std::string ty = val.substr(0, colon);
        q.type = ty == "f32" ? 0 : ty == "f16" ? 1 : ty == "i32" ? 26 : ty[0] == 't' ? atoi(ty.c_str() + 1) : -1;
        if (q.type < 0) return false;
        std::string rest = val.substr(colon + 1), addr, nb;
        size_t at = rest.find('@');
        if (at != std::string::npos) { addr = rest.substr(at + 1); rest = rest.substr(0, at); }
        size_t sl = rest.find('/');
        if (sl != std::string::npos) { nb = rest.substr(sl + 1); rest = rest.substr(0, sl); }
        for (int i = 0; i < 4; ++i) q.ne[i] = 1;
        { std::istringstream e(rest); std::string x; int i = 0; while (std::getline(e, x, ',') && i < 4) q.ne[i++] = atoll(x.c_str()); }
        const bool quant = q.type != 0 && q.type != 1 && q.type != 26;
        q.nb[0] = quant ? qmm::type_tsize(q.type) : q.type == 1 ? 2 : 4;
        q.nb[1] = quant ? q.ne[0] / qmm::type_blck(q.type) * q.nb[0] : q.nb[0] * q.ne[0];
        q.nb[2] = q.nb[1] * q.ne[1];
        q.nb[3] = q.nb[2] * q.ne[2];
        if (!nb.empty()) { std::istringstream e(nb); std::string x; int i = 0; while (std::getline(e, x, ',') && i < 4) q.nb[i++] = atoll(x.c_str()); }
        q.data = (void *) (uintptr_t) (addr.empty() ? (uint64_t) (++slot) << 20 : strtoull(addr.c_str(), nullptr, 0));
        if (addr.empty() == false) ++slot;
        s.t[name] = q;
    }
    for (const char * dn : { "d", "qd" }) {
        auto it = s.t.find(dn);
        if (it != s.t.end()) for (int i = 0; i < 16; ++i) if (pset[i]) it->second.op_params[i] = pi[i];
    }
    return true;
}
static int op_id(const std::string & n) {
    static const char * names[] = { "", "ADD", "SUB", "MUL", "DIV", "SCALE", "SILU", "GELU", "GELU_QUICK", "RELU", "TANH", "SIGMOID", "NEG", "EXP", "RMS_NORM", "ROPE",
                                    "SOFT_MAX", "CPY", "GET_ROWS", "MUL_MAT_F", "RMS_NORM_MUL", "SILU_MUL", "ARGSORT", "SUM_ROWS", "NORM" };
    for (int i = 1; i < (int) (sizeof(names) / sizeof(names[0])); ++i) if (n == names[i]) return i;
    return 0;
}
using namespace qmm;
int main() {
    static const struct { const char * name; int nargs; } KERNELS[GK_COUNT] = {
        { "none", 0 }, { "binary_kernel", 2 }, { "unary_kernel", 2 }, { "rms_norm_kernel", 1 }, { "rms_norm_vec_kernel", 3 }, { "norm_kernel", 0 },
        { "soft_max_wave_kernel", 1 }, { "soft_max_kernel", 1 }, { "rope_kernel", 0 }, { "memcpy", 0 }, { "cpy_kernel", 2 }, { "cpy_transpose_kernel", 2 },
        { "get_rows_kernel", 1 }, { "get_rows_q_kernel", 1 }, { "mul_mat_f16_kernel", 1 }, { "mul_mat_dot_block_kernel", 0 }, { "mul_mat_dot_kernel", 1 },
        { "argsort_kernel", 0 }, { "sum_rows_kernel", 0 }, { "rope_store_kernel", 1 }, { "moe_router_kernel", 0 }, { "moe_router_logits_kernel", 1 },
        { "moe_combine_kernel", 0 }, { "moe_combine_add_norm_kernel", 1 } };
    std::string line;
    while (std::getline(std::cin, line)) {
        Spec s;
        if (!parse_spec(line, s)) { fprintf(stderr, "bad spec: %s\n", line.c_str()); return 1; }
        auto T = [&](const char * n) { return s.get(n); };
        bool sup;
        GluePlan p;
        if (s.entry.compare(0, 3, "op:") == 0) {
            const int op = op_id(s.entry.substr(3));
            if ((sup = sup_op(op, T("a"), T("b"), T("c"), T("d")))) p = glue_op_plan(op, T("a"), T("b"), T("c"), T("d"));
        } else if (s.entry == "add_rms_norm") {
            if ((sup = sup_add_rms_norm(T("a"), T("b"), T("w"), T("sum"), T("d")))) p = glue_add_rms_norm_plan(T("a"), T("b"), T("w"), T("sum"), T("d"));
        } else if (s.entry == "rope_store") {
            if ((sup = sup_rope_kv_store(T("q"), T("pos"), T("ff"), T("qd"), T("k"), T("kd"), T("v"), T("vd")))) p = glue_rope_kv_store_plan(T("q"), T("k"), T("v"), T("vd"));
        } else if (s.entry == "router") {
            if ((sup = sup_moe_router(T("logits"), T("ids"), T("weights"), s.n_used))) p = glue_moe_router_plan(T("logits"));
        } else if (s.entry == "router_logits") {
            if ((sup = sup_moe_router_logits(T("gate"), T("x"), T("logits"), T("ids"), T("weights"), s.n_used))) p = glue_moe_router_logits_plan(T("x"), false);
        } else if (s.entry == "router_logits_norm") {
            if ((sup = sup_moe_router_logits_norm(T("gate"), T("x"), T("nw"), T("normed"), T("logits"), T("ids"), T("weights"), s.n_used))) p = glue_moe_router_logits_plan(T("x"), true);
        } else if (s.entry == "combine") {
            if ((sup = sup_moe_combine(T("x"), T("w"), T("out")))) p = glue_moe_combine_plan(T("x"), T("out"));
        } else if (s.entry == "combine_add_rms_norm") {
            if ((sup = sup_moe_combine_add_rms_norm(T("x"), T("w"), T("b"), T("nw"), T("sum"), T("d")))) p = glue_moe_combine_add_rms_norm_plan(T("x"));
        } else { fprintf(stderr, "bad entry: %s\n", line.c_str()); return 1; }
        if (!sup) { printf("unsupported\n"); continue; }
        char label[96] = "none", kernel[96] = "none";
        if (p.label) snprintf(label, sizeof(label), p.label, p.targ[0]);          // as QMM_TRACE formats it, while tracing
        if (p.launch) {
            int n = snprintf(kernel, sizeof(kernel), "%s", KERNELS[p.kernel].name);
            for (int i = 0; i < KERNELS[p.kernel].nargs; ++i) n += snprintf(kernel + n, sizeof(kernel) - n, "%s%d", i ? "," : "<", p.targ[i]);
            if (KERNELS[p.kernel].nargs) snprintf(kernel + n, sizeof(kernel) - n, ">");
        }
        printf("%s %s grid=%u,%u,%u block=%u lds=%zu karg=%u,%u ", label, kernel, p.grid[0], p.grid[1], p.grid[2], p.block, p.lds, p.karg[0], p.karg[1]);
        if (p.err) printf("%d:%s\n", p.err, p.msg); else printf("ok\n");
    }
    return 0;
}
"""
# (operands of one entry point, what the launch code did with them before the plan existed).  A spec: the entry point ("op:NAME" is qmm_op_compute),
# then its operands by name as TYPE:extents[/byte strides][@address]; strides default to contiguous, addresses to 1 MiB slots; pi<i> / pf<i> set
# op_params of the destination (rope: n_dims and mode, soft_max: scale and max_bias).  A result: trace label, instantiation (bools 0 / 1, element
# types by their ids; none: nothing was launched or copied), grid, block, dynamic LDS bytes, the two grid-derived arguments of rope_store_kernel<1>,
# then ok or the refusal's code and text; or "unsupported" where the entry point's support predicate turns the operands away.  The right-hand sides were printed by the launch code of the commit before this header (the support
# predicates, the launch_* functions and every entry point of qmm_ops.hip) copied into a stand-alone program with each launch replaced by a
# print, never by the header.  Every branch of every ladder on both sides of its boundary, one condition at a time.
GLUE_PLAN_TABLE = [
    ("op:ADD a=f32:4096,512 b=f32:4096 d=f32:4096,512",
     "binary_kernel<vec> binary_kernel<1,1> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4098,3/4,16400,49200,49200 b=f32:4098/4,16400,16400,16400 d=f32:4098,3/4,16400,49200,49200",
     "binary_kernel<scalar> binary_kernel<1,0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4100,3/4,16400,49200,49200 b=f32:4100/4,16400,16400,16400 d=f32:4100,3/4,16400,49200,49200",
     "binary_kernel<vec> binary_kernel<1,1> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512 b=f32:1,512/4,16,8192,8192 d=f32:4096,512",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512 b=f32:4096/8,32768,32768,32768 d=f32:4096,512",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512@0x100004 b=f32:4096 d=f32:4096,512",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512 b=f32:4096@0x200004 d=f32:4096,512",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512 b=f32:4096 d=f32:4096,512@0x300004",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512/4,16388,8390656,8390656 b=f32:4096 d=f32:4096,512",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512 b=f32:4096,512/4,16388,8390656,8390656 d=f32:4096,512",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ADD a=f32:4096,512 b=f32:4096 d=f32:4096,512/4,16388,8390656,8390656",
     "binary_kernel<scalar> binary_kernel<1,0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:1020,7 b=f32:1020,7 d=f32:1020,7",
     "binary_kernel<vec> binary_kernel<3,1> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:1024,7 b=f32:1024,7 d=f32:1024,7",
     "binary_kernel<vec> binary_kernel<3,1> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:1028,7 b=f32:1028,7 d=f32:1028,7",
     "binary_kernel<vec> binary_kernel<3,1> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:255,7@0x100004 b=f32:255,7 d=f32:255,7",
     "binary_kernel<scalar> binary_kernel<3,0> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:256,7@0x100004 b=f32:256,7 d=f32:256,7",
     "binary_kernel<scalar> binary_kernel<3,0> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:257,7@0x100004 b=f32:257,7 d=f32:257,7",
     "binary_kernel<scalar> binary_kernel<3,0> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:512,7 b=f32:512 d=f32:512,7",
     "binary_kernel<vec> binary_kernel<3,1> grid=4,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:516,7 b=f32:516 d=f32:516,7",
     "binary_kernel<vec> binary_kernel<3,1> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:128,7@0x100004 b=f32:128 d=f32:128,7",
     "binary_kernel<scalar> binary_kernel<3,0> grid=4,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL a=f32:129,7 b=f32:129 d=f32:129,7",
     "binary_kernel<scalar> binary_kernel<3,0> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SUB a=f32:64,35 b=f32:64 d=f32:64,35",
     "binary_kernel<vec> binary_kernel<2,1> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:DIV a=f32:5,103 b=f32:5,103 d=f32:5,103",
     "binary_kernel<scalar> binary_kernel<4,0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SUB a=f32:5,103 b=f32:1 d=f32:5,103",
     "binary_kernel<scalar> binary_kernel<2,0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:DIV a=f32:64,5,7 b=f32:64,1,7 d=f32:64,5,7",
     "binary_kernel<vec> binary_kernel<4,1> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SILU a=f32:0 d=f32:0",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 ok"),
    ("op:SILU a=f32:1 d=f32:1",
     "unary_kernel unary_kernel<6,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SILU a=f32:1024 d=f32:1024",
     "unary_kernel unary_kernel<6,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SILU a=f32:1025 d=f32:1025",
     "unary_kernel unary_kernel<6,0> grid=2,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SCALE a=f32:4096,3 d=f32:4096,3",
     "unary_kernel unary_kernel<5,0> grid=12,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:EXP a=f32:4096,3 d=f32:4096,3",
     "unary_kernel unary_kernel<13,0> grid=12,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SILU_MUL a=f32:4100,3 b=f32:4100,3 d=f32:4100,3",
     "unary_kernel unary_kernel<6,1> grid=13,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SILU_MUL a=f32:0 b=f32:0 d=f32:0",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4096,256 d=f32:4096,256",
     "rms_norm_vec_kernel<256> rms_norm_vec_kernel<0,0,256> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:4096,256 b=f32:4096 d=f32:4096,256",
     "rms_norm_vec_kernel<256> rms_norm_vec_kernel<1,0,256> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4100,256 d=f32:4100,256",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<0,0,1024> grid=256,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:4100,256 b=f32:4100 d=f32:4100,256",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,0,1024> grid=256,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4096,255 d=f32:4096,255",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<0,0,1024> grid=255,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:4096,255 b=f32:4096 d=f32:4096,255",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,0,1024> grid=255,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:16384,3 d=f32:16384,3",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<0,0,1024> grid=3,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:16384,3 b=f32:16384 d=f32:16384,3",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,0,1024> grid=3,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:16388,3 d=f32:16388,3",
     "rms_norm_kernel rms_norm_kernel<0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:16388,3 b=f32:16388 d=f32:16388,3",
     "rms_norm_kernel rms_norm_kernel<1> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4098,3 d=f32:4098,3",
     "rms_norm_kernel rms_norm_kernel<0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:4098,3 b=f32:4098 d=f32:4098,3",
     "rms_norm_kernel rms_norm_kernel<1> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:16384,256 d=f32:16384,256",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<0,0,1024> grid=256,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:16384,256 b=f32:16384 d=f32:16384,256",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,0,1024> grid=256,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4096,3@0x100004 d=f32:4096,3",
     "rms_norm_kernel rms_norm_kernel<0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4096,3 d=f32:4096,3@0x200004",
     "rms_norm_kernel rms_norm_kernel<0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:4096,3 b=f32:4096@0x200004 d=f32:4096,3",
     "rms_norm_kernel rms_norm_kernel<1> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4096,3/4,16388,49164,49164 d=f32:4096,3",
     "rms_norm_kernel rms_norm_kernel<0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4098,3/4,16400,49200,49200 d=f32:4098,3/4,16400,49200,49200",
     "rms_norm_kernel rms_norm_kernel<0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:4098,3/4,16400,49200,49200 b=f32:4098 d=f32:4098,3/4,16400,49200,49200",
     "rms_norm_kernel rms_norm_kernel<1> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM a=f32:4100,3/4,16400,49200,49200 d=f32:4100,3/4,16400,49200,49200",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<0,0,1024> grid=3,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("op:RMS_NORM_MUL a=f32:4096,300 b=f32:4096 d=f32:4096,300/4,16388,4916400,4916400",
     "rms_norm_kernel rms_norm_kernel<1> grid=300,1,1 block=256 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:4096,1 b=f32:4096,1 w=f32:4096 sum=f32:4096,1 d=f32:4096,1",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,1,1024> grid=1,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:4096,255 b=f32:4096,255 w=f32:4096 sum=f32:4096,255 d=f32:4096,255",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,1,1024> grid=255,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:4096,256 b=f32:4096,256 w=f32:4096 sum=f32:4096,256 d=f32:4096,256",
     "rms_norm_vec_kernel<256> rms_norm_vec_kernel<1,1,256> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:4100,256 b=f32:4100,256 w=f32:4100 sum=f32:4100,256 d=f32:4100,256",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,1,1024> grid=256,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:16384,2 b=f32:16384,2 w=f32:16384 sum=f32:16384,2 d=f32:16384,2",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,1,1024> grid=2,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:4096,256 b=f32:4096,256 sum=f32:4096,256 d=f32:4096,256",
     "rms_norm_vec_kernel<256> rms_norm_vec_kernel<0,1,256> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:4096,2 b=f32:4096,2 w=f32:4096 sum=f32:4096,2@0x400004 d=f32:4096,2",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 -5:ADD + RMS_NORM: rows must be 16-byte aligned, ne0 % 4 == 0 and ne0 <= 16384"),
    ("add_rms_norm a=f32:4096,2 b=f32:4096,2@0x200004 w=f32:4096 sum=f32:4096,2 d=f32:4096,2",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 -5:ADD + RMS_NORM: rows must be 16-byte aligned, ne0 % 4 == 0 and ne0 <= 16384"),
    ("add_rms_norm a=f32:4096,2@0x100004 b=f32:4096,2 sum=f32:4096,2 d=f32:4096,2",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 -5:ADD + RMS_NORM: rows must be 16-byte aligned, ne0 % 4 == 0 and ne0 <= 16384"),
    ("add_rms_norm a=f32:4096,2 b=f32:4096,2 w=f32:4096@0x300004 sum=f32:4096,2 d=f32:4096,2",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 -5:ADD + RMS_NORM: rows must be 16-byte aligned, ne0 % 4 == 0 and ne0 <= 16384"),
    ("add_rms_norm a=f32:4096,2 b=f32:4096,2 w=f32:4096 sum=f32:4096,2 d=f32:4096,2@0x500004",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 -5:ADD + RMS_NORM: rows must be 16-byte aligned, ne0 % 4 == 0 and ne0 <= 16384"),
    ("add_rms_norm a=f32:4100,3/4,16400,49200,49200 b=f32:4100,3/4,16400,49200,49200 w=f32:4100 sum=f32:4100,3/4,16400,49200,49200 d=f32:4100,3/4,16400,49200,49200",
     "rms_norm_vec_kernel<1024> rms_norm_vec_kernel<1,1,1024> grid=3,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("add_rms_norm a=f32:4098,3/4,16400,49200,49200 b=f32:4098,3/4,16400,49200,49200 w=f32:4098 sum=f32:4098,3/4,16400,49200,49200 d=f32:4098,3/4,16400,49200,49200",
     "unsupported"),
    ("add_rms_norm a=f32:16388,3 b=f32:16388,3 w=f32:16388 sum=f32:16388,3 d=f32:16388,3",
     "unsupported"),
    ("op:NORM a=f32:100,7,3 d=f32:100,7,3",
     "norm_kernel norm_kernel grid=21,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ROPE a=f32:66,3,5 b=i32:5 d=f32:66,3,5 pi1=64 pi2=2",
     "rope_kernel rope_kernel grid=2,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ROPE a=f32:128,32,4 b=i32:4 c=f32:64 d=f32:128,32,4 pi1=128 pi2=0",
     "rope_kernel rope_kernel grid=32,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:ARGSORT a=f32:100,7 d=i32:100,7 pi0=1",
     "argsort_kernel argsort_kernel grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SUM_ROWS a=f32:100,7 d=f32:1,7",
     "sum_rows_kernel sum_rows_kernel grid=2,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SUM_ROWS a=f32:100,8 d=f32:1,8",
     "sum_rows_kernel sum_rows_kernel grid=2,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,32,32 b=f32:256,32 d=f32:256,32,32",
     "soft_max_wave_kernel<1> soft_max_wave_kernel<1> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:260,32,32 b=f32:260,32 d=f32:260,32,32",
     "soft_max_wave_kernel<2> soft_max_wave_kernel<2> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:512,32,32 b=f32:512,32 d=f32:512,32,32",
     "soft_max_wave_kernel<2> soft_max_wave_kernel<2> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:516,32,32 b=f32:516,32 d=f32:516,32,32",
     "soft_max_wave_kernel<4> soft_max_wave_kernel<4> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:1024,32,32 b=f32:1024,32 d=f32:1024,32,32",
     "soft_max_wave_kernel<4> soft_max_wave_kernel<4> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:1028,32,32 b=f32:1028,32 d=f32:1028,32,32",
     "soft_max_kernel<lds> soft_max_kernel<0> grid=1024,1,1 block=256 lds=4112 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,1023 d=f32:256,1023",
     "soft_max_kernel<lds> soft_max_kernel<0> grid=1023,1,1 block=256 lds=1024 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,1024 d=f32:256,1024",
     "soft_max_wave_kernel<1> soft_max_wave_kernel<1> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,1025 d=f32:256,1025",
     "soft_max_wave_kernel<1> soft_max_wave_kernel<1> grid=257,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:254,32,32 b=f32:254,32 d=f32:254,32,32",
     "soft_max_kernel<lds> soft_max_kernel<0> grid=1024,1,1 block=256 lds=1016 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,32,32 b=f32:256,32 d=f32:256,32,32 pf0=0.125 pf1=8",
     "soft_max_kernel<lds> soft_max_kernel<0> grid=1024,1,1 block=256 lds=1024 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,32,32 b=f16:256,32 d=f32:256,32,32",
     "soft_max_kernel<lds> soft_max_kernel<1> grid=1024,1,1 block=256 lds=1024 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,32,32 b=f32:256,32@0x200004 d=f32:256,32,32",
     "soft_max_kernel<lds> soft_max_kernel<0> grid=1024,1,1 block=256 lds=1024 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,32,32@0x100004 b=f32:256,32 d=f32:256,32,32",
     "soft_max_kernel<lds> soft_max_kernel<0> grid=1024,1,1 block=256 lds=1024 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:256,32,32 b=f32:256,32 d=f32:256,32,32@0x300004",
     "soft_max_kernel<lds> soft_max_kernel<0> grid=1024,1,1 block=256 lds=1024 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:8192,3 b=f16:8192,3 d=f32:8192,3",
     "soft_max_kernel<lds> soft_max_kernel<1> grid=3,1,1 block=256 lds=32768 karg=0,0 ok"),
    ("op:SOFT_MAX a=f32:8196,3 b=f32:8196,4 d=f32:8196,3",
     "soft_max_kernel<dst> soft_max_kernel<0> grid=3,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:64,64 d=f32:64,64",
     "memcpy memcpy grid=0,0,0 block=0 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:64,64@0x100000 d=f16:64,64@0x100000",
     "memcpy none grid=0,0,0 block=0 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:64,64@0x100000 d=f32:4096@0x100000",
     "memcpy none grid=0,0,0 block=0 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:64,64/4,512,32768,32768 d=f32:64,64",
     "cpy_kernel cpy_kernel<0,0> grid=16,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:10,10,10 d=f32:1000",
     "cpy_kernel cpy_kernel<1,0> grid=4,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:0 d=f16:0",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:32,8/32,4,1024,1024 d=f32:32,8",
     "cpy_transpose_kernel cpy_transpose_kernel<0,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:32,8/32,4,1024,1024 d=f16:32,8",
     "cpy_transpose_kernel cpy_transpose_kernel<0,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:32,8/16,2,512,512 d=f32:32,8",
     "cpy_transpose_kernel cpy_transpose_kernel<1,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:32,8/16,2,512,512 d=f16:32,8",
     "cpy_transpose_kernel cpy_transpose_kernel<1,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:31,8/32,4,992,992 d=f32:31,8",
     "cpy_kernel cpy_kernel<0,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:31,8/32,4,992,992 d=f16:31,8",
     "cpy_kernel cpy_kernel<0,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:31,8/16,2,496,496 d=f32:31,8",
     "cpy_kernel cpy_kernel<1,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:31,8/16,2,496,496 d=f16:31,8",
     "cpy_kernel cpy_kernel<1,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:32,7/28,4,896,896 d=f32:32,7",
     "cpy_kernel cpy_kernel<0,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:32,7/14,2,448,448 d=f32:32,7",
     "cpy_kernel cpy_kernel<1,0> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f16:32,7/14,2,448,448 d=f16:32,7",
     "cpy_kernel cpy_kernel<1,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:32,8/32,4,1024,1024 d=f16:32,8/4,128,1024,1024",
     "cpy_kernel cpy_kernel<0,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:32,7/28,4,896,896 d=f16:32,7",
     "cpy_kernel cpy_kernel<0,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:1024,70/280,4,286720,286720 d=f16:1024,70/2,4096,286720,286720",
     "cpy_transpose_kernel cpy_transpose_kernel<0,1> grid=32,3,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:32,8,2/32,4,1024,2048 d=f16:32,8,2",
     "cpy_kernel cpy_kernel<0,1> grid=2,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:CPY a=f32:32,8/64,8,2048,2048 d=f16:32,8",
     "cpy_kernel cpy_kernel<0,1> grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:GET_ROWS a=f32:64,100 b=i32:7 d=f32:64,7",
     "get_rows_kernel get_rows_kernel<0> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:GET_ROWS a=f16:64,100,2 b=i32:7,2 d=f32:64,7,2",
     "get_rows_kernel get_rows_kernel<1> grid=14,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:GET_ROWS a=t12:4096,100 b=i32:7 d=f32:4096,7",
     "get_rows_q_kernel<12> get_rows_q_kernel<12> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:GET_ROWS a=t8:4096,100 b=i32:300 d=f32:4096,300",
     "get_rows_q_kernel<8> get_rows_q_kernel<8> grid=300,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f16:64,70,2 b=f32:64,65,4 d=f32:70,65,4",
     "mul_mat_f16_kernel<vec> mul_mat_f16_kernel<1> grid=2,2,4 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f16:64,70,2@0x100004 b=f32:64,65,4 d=f32:70,65,4",
     "mul_mat_f16_kernel<scalar> mul_mat_f16_kernel<0> grid=2,2,4 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f16:64,70,2/2,136,9520,19040 b=f32:64,65,4 d=f32:70,65,4",
     "mul_mat_f16_kernel<scalar> mul_mat_f16_kernel<0> grid=2,2,4 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f16:64,70,2 b=f32:64,65,4@0x200004 d=f32:70,65,4",
     "mul_mat_f16_kernel<scalar> mul_mat_f16_kernel<0> grid=2,2,4 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f16:64,70,2 b=f32:64,65,4/4,260,16900,67600 d=f32:70,65,4",
     "mul_mat_f16_kernel<scalar> mul_mat_f16_kernel<0> grid=2,2,4 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f16:64,70,2 b=f32:64,65,4 d=f32:70,65,4@0x300004",
     "mul_mat_f16_kernel<vec> mul_mat_f16_kernel<1> grid=2,2,4 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f16:128,640,8/2,2048,256,1310720 b=f32:128,512,32/4,16384,512,8388608 d=f32:640,512,32",
     "mul_mat_f16_kernel<vec> mul_mat_f16_kernel<1> grid=10,8,32 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f32:1024,2048 b=f32:1024,1 d=f32:2048,1",
     "mul_mat_dot_block_kernel mul_mat_dot_block_kernel grid=2048,1,1 block=128 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f32:1024,2049 b=f32:1024,1 d=f32:2049,1",
     "mul_mat_dot_kernel mul_mat_dot_kernel<0> grid=513,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f32:1023,2048 b=f32:1023,1 d=f32:2048,1",
     "mul_mat_dot_kernel mul_mat_dot_kernel<0> grid=512,1,1 block=256 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f32:1024,8 b=f32:1024,3,2,2 d=f32:8,3,2,2",
     "mul_mat_dot_block_kernel mul_mat_dot_block_kernel grid=24,1,4 block=128 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f32:4096,8 b=f32:4096,1 d=f32:8,1",
     "mul_mat_dot_block_kernel mul_mat_dot_block_kernel grid=8,1,1 block=128 lds=0 karg=0,0 ok"),
    ("op:MUL_MAT_F a=f32:64,9,2 b=f32:64,5,4 d=f32:9,5,4",
     "mul_mat_dot_kernel mul_mat_dot_kernel<0> grid=12,1,4 block=256 lds=0 karg=0,0 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0 k=f32:128,8,4 kd=f16:128,8,4 v=f32:32,32/128,4,4096,4096 vd=f16:32,32",
     "none rope_store_kernel<1> grid=6,1,1 block=256 lds=0 karg=5,1 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0 k=f32:128,8,4 kd=f16:128,8,4 v=f32:31,32/128,4,3968,3968 vd=f16:31,32",
     "none rope_store_kernel<0> grid=9,1,1 block=256 lds=0 karg=0,0 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0 k=f32:128,8,4 kd=f16:128,8,4 v=f32:32,31/124,4,3968,3968 vd=f16:32,31",
     "none rope_store_kernel<0> grid=9,1,1 block=256 lds=0 karg=0,0 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0 k=f32:128,8,4 kd=f16:128,8,4 v=f32:1024,70/280,4,286720,286720 vd=f16:1024,70",
     "none rope_store_kernel<1> grid=101,1,1 block=256 lds=0 karg=5,32 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0 v=f32:32,32/128,4,4096,4096 vd=f16:32,32",
     "none rope_store_kernel<1> grid=5,1,1 block=256 lds=0 karg=4,1 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0 k=f32:128,8,4 kd=f16:128,8,4",
     "none rope_store_kernel<0> grid=5,1,1 block=256 lds=0 karg=0,0 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0",
     "none rope_store_kernel<0> grid=4,1,1 block=256 lds=0 karg=0,0 ok"),
    ("rope_store q=f32:128,12,3 pos=i32:3 ff=f32:32 qd=f32:128,12,3 pi1=64 pi2=2 k=f32:128,3,3 kd=f16:128,3,3 v=f32:384,3 vd=f16:3,384",
     "none rope_store_kernel<0> grid=7,1,1 block=256 lds=0 karg=0,0 ok"),
    ("rope_store q=f32:128,32,4 pos=i32:4 qd=f32:128,32,4 pi1=128 pi2=0 k=f32:128,8,4 kd=f16:128,8,4 v=f32:1024,4 vd=f16:4,1024/2,8192,8388608,8388608",
     "none rope_store_kernel<0> grid=21,1,1 block=256 lds=0 karg=0,0 ok"),
    ("router logits=f32:8,1 ids=i32:8,1 weights=f32:2,1 n_used=2",
     "none moe_router_kernel grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("router logits=f32:8,4 ids=i32:8,4 weights=f32:2,4 n_used=2",
     "none moe_router_kernel grid=1,1,1 block=256 lds=0 karg=0,0 ok"),
    ("router logits=f32:8,5 ids=i32:8,5 weights=f32:2,5 n_used=2",
     "none moe_router_kernel grid=2,1,1 block=256 lds=0 karg=0,0 ok"),
    ("router logits=f32:64,512 ids=i32:64,512 weights=f32:6,512 n_used=6",
     "none moe_router_kernel grid=128,1,1 block=256 lds=0 karg=0,0 ok"),
    ("router_logits gate=f32:4096,8 x=f32:4096,1 logits=f32:8,1 ids=i32:8,1 weights=f32:2,1 n_used=2",
     "none moe_router_logits_kernel<0> grid=1,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("router_logits gate=f32:1024,8 x=f32:1024,8 logits=f32:8,8 ids=i32:8,8 weights=f32:2,8 n_used=2",
     "none moe_router_logits_kernel<0> grid=8,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("router_logits_norm gate=f32:4096,8 x=f32:4096,1 nw=f32:4096 normed=f32:4096,1 logits=f32:8,1 ids=i32:8,1 weights=f32:2,1 n_used=2",
     "none moe_router_logits_kernel<1> grid=1,1,1 block=1024 lds=16384 karg=0,0 ok"),
    ("router_logits_norm gate=f32:16384,8 x=f32:16384,8 nw=f32:16384 normed=f32:16384,8 logits=f32:8,8 ids=i32:8,8 weights=f32:2,8 n_used=2",
     "none moe_router_logits_kernel<1> grid=8,1,1 block=1024 lds=65536 karg=0,0 ok"),
    ("router_logits_norm gate=f32:4098,8/4,16400,131200,131200 x=f32:4098,1/4,16400,16400,16400 nw=f32:4098 normed=f32:4098,1/4,16400,16400,16400 logits=f32:8,1 ids=i32:8,1 weights=f32:2,1 n_used=2",
     "unsupported"),
    ("router_logits_norm gate=f32:4100,8 x=f32:4100,1 nw=f32:4100 normed=f32:4100,1 logits=f32:8,1 ids=i32:8,1 weights=f32:2,1 n_used=2",
     "none moe_router_logits_kernel<1> grid=1,1,1 block=1024 lds=16400 karg=0,0 ok"),
    ("combine x=f32:1024,2,3 w=f32:1,2,3 out=f32:1024,3",
     "none moe_combine_kernel grid=1,3,1 block=256 lds=0 karg=0,0 ok"),
    ("combine x=f32:1028,2,3 w=f32:1,2,3 out=f32:1028,3",
     "none moe_combine_kernel grid=2,3,1 block=256 lds=0 karg=0,0 ok"),
    ("combine x=f32:4096,2,1@0x100004 w=f32:1,2,1 out=f32:4096,1",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 -1:qmm_moe_combine: x / out must be 16-byte aligned"),
    ("combine x=f32:4096,2,1 w=f32:1,2,1 out=f32:4096,1@0x300004",
     "none none grid=0,0,0 block=0 lds=0 karg=0,0 -1:qmm_moe_combine: x / out must be 16-byte aligned"),
    ("combine_add_rms_norm x=f32:4096,2,1 w=f32:1,2,1 b=f32:4096,1 nw=f32:4096 sum=f32:4096,1 d=f32:4096,1",
     "none moe_combine_add_norm_kernel<1024> grid=1,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("combine_add_rms_norm x=f32:4096,2,255 w=f32:1,2,255 b=f32:4096,255 nw=f32:4096 sum=f32:4096,255 d=f32:4096,255",
     "none moe_combine_add_norm_kernel<1024> grid=255,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("combine_add_rms_norm x=f32:4096,2,256 w=f32:1,2,256 b=f32:4096,256 nw=f32:4096 sum=f32:4096,256 d=f32:4096,256",
     "none moe_combine_add_norm_kernel<256> grid=256,1,1 block=256 lds=0 karg=0,0 ok"),
    ("combine_add_rms_norm x=f32:4100,2,256 w=f32:1,2,256 b=f32:4100,256 nw=f32:4100 sum=f32:4100,256 d=f32:4100,256",
     "none moe_combine_add_norm_kernel<1024> grid=256,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("combine_add_rms_norm x=f32:16384,2,256 w=f32:1,2,256 b=f32:16384,256 nw=f32:16384 sum=f32:16384,256 d=f32:16384,256",
     "none moe_combine_add_norm_kernel<1024> grid=256,1,1 block=1024 lds=0 karg=0,0 ok"),
    ("combine_add_rms_norm x=f32:16388,2,2 w=f32:1,2,2 b=f32:16388,2 nw=f32:16388 sum=f32:16388,2 d=f32:16388,2",
     "unsupported"),
]


@pytest.fixture(scope="module")
def glue_plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each operand spec on its input"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("glueplan")
    (d / "probe.cpp").write_text(GLUE_PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{GLUE_PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_glue_plan_keeps_every_decision(glue_plan_probe):
    assert len(GLUE_PLAN_TABLE) >= 80
    got = glue_plan_probe([spec for spec, _ in GLUE_PLAN_TABLE])
    assert len(got) == len(GLUE_PLAN_TABLE)
    for (spec, want), line in zip(GLUE_PLAN_TABLE, got):
        assert line == want, spec


def test_glue_rules_live_in_one_place():
    """the plan functions, the support predicates and the rules two kernels share are defined in the plan header only; a glue kernel is launched
    only by run_glue of qmm_ops.hip; one QMM_TRACE serves the glue launches, in run_glue (comments may speak of all this)"""
    def code_of(f):
        return [re.sub(r"//.*$", "", line) for line in f.read_text().splitlines()]
    defines = re.compile(r"\b(?:GluePlan|bool|int)\s+(glue_\w*plan|sup_\w+|row_norm_\w+|transpose_2d)\s*\(")
    found = sorted(m.group(1) for line in code_of(GLUE_PLAN_HEADER) for m in defines.finditer(line))
    assert len(found) == len(set(found))
    for name in ("glue_op_plan", "glue_add_rms_norm_plan", "glue_rope_kv_store_plan", "glue_moe_router_plan", "glue_moe_router_logits_plan", "glue_moe_combine_plan",
                 "glue_moe_combine_add_rms_norm_plan", "sup_op", "sup_add_rms_norm", "sup_rope_kv_store", "sup_moe_router", "sup_moe_router_logits",
                 "sup_moe_router_logits_norm", "sup_moe_combine", "sup_moe_combine_add_rms_norm", "row_norm_threads", "row_norm_in_regs", "transpose_2d"):
        assert name in found, name
    kernels = set()                                                          # every __global__ function of the unit that is not of the attention section
    unit = code_of(GLUE_UNIT)
    for n, line in enumerate(unit):
        if "__global__" in line:
            kernels.update(re.findall(r"^(\w+_kernel)\s*\(", unit[n + 1]))
    assert len(kernels) >= 22, sorted(kernels)
    launch = re.compile(r"hipLaunchKernelGGL\s*\((.*)$")
    traces = 0
    for f in sorted((ROOT / "ggml-hexagon_amd" / "csrc").iterdir()):
        if f.suffix not in (".cpp", ".h", ".hip", ".hiph"):
            continue
        inside = None                                                        # the function a line belongs to: the last line that opened one at column 0
        for n, line in enumerate(code_of(f), 1):
            where = f"{f.name}:{n}: {line.strip()[:120]}"
            if re.match(r"^\w.*\)\s*\{", line):
                inside = line
            if f != GLUE_PLAN_HEADER:
                assert not defines.search(line), where
                assert not re.search(r"rows\s*<\s*256|>\s*256\s*\*\s*16|<=\s*1024\s*\*\s*16", line), where          # the row-norm rules, spelled out
            m = launch.search(line)
            if m and (f == GLUE_UNIT or any(re.search(rf"\b{k}\b", m.group(1)) for k in kernels)):
                assert f == GLUE_UNIT and inside is not None and re.search(r"\brun_glue\s*\(", inside), where
            if f == GLUE_UNIT and "QMM_TRACE" in line:
                traces += 1
                assert inside is not None and re.search(r"\brun_glue\s*\(", inside), where
    assert traces == 1
