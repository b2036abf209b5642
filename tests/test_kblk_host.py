"""CPU-side tests of a K cache in Q4_0, Q4_1, Q5_0 or Q5_1 (llama.cpp's -ctk q4_0 / q4_1 / q5_0 / q5_1 without flash attention;
csrc/qmm_kblk_plan.h, csrc/qmm_kblk.hiph): the numpy restatement of the four quantizers (tests/kblk_refs.py) against the reference's bytes in
tests/golden/kblk_quantize.npz and, where oracle/_ref is built, against the live reference; the launch plans through a probe the host
compiler builds from the plan header alone; and what the entry points of include/ggml_mi355x_ops.h take with a tensor of such a type among
their operands, through the library loaded without a device."""
import ctypes
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import kblk_refs as R  # noqa: E402

PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_kblk_plan.h"
TYPE_IDS = [R.NAMES[t] for t in R.TYPES]


# ---- the restatement

@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_restatement_gives_the_golden_bytes(t):
    g = R.load_golden()
    a, b = R.golden_inputs()
    assert np.array_equal(a, g["a"]) and np.array_equal(b, g["b"])                       # the file's rows are the rows the GPU tests copy
    for s in "ab":
        want = g[f"{s}_{R.NAMES[t]}"]
        assert want.dtype == np.uint8 and want.shape == (g[s].shape[0], g[s].shape[1] // 32 * R.BLOCK[t])
        got = R.quantize(t, g[s])
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    # the edges are in the file: a block of d = 0, a code on the clamp, and for the _1 types an m that f16 rounds
    blocks = np.concatenate([g[f"a_{R.NAMES[t]}"].reshape(-1, R.BLOCK[t]), g[f"b_{R.NAMES[t]}"].reshape(-1, R.BLOCK[t])])
    d, m = R.scales(t, blocks)
    assert ((d & 0x7FFF) == 0).any() and (R.codes(t, blocks) == (31 if R.HAS_QH[t] else 15)).any()
    if R.HAS_M[t]:
        mins = np.concatenate([g["a"].reshape(-1, 32), g["b"].reshape(-1, 32)]).min(axis=1)
        assert (m.view(np.float16).astype(np.float32) != mins).any()


@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_restatement_is_the_live_reference(t):
    from oracle.pyoracle import RefGgml, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref is not built (it needs the reference tree at build time)")
    ref = RefGgml()
    x = np.random.default_rng(t).normal(0, 1, (96, 256)).astype(np.float32)
    x[::7] *= 30.0
    w = ref.quantize_weights(t, x)
    assert np.array_equal(R.quantize(t, x), w)
    assert np.array_equal(R.dequantize(t, w, 256), ref.dequantize(t, w, 256))


@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_restated_dequantizer_is_the_oracle(t):
    from oracle.pyoracle import Oracle
    g = R.load_golden()
    w = g[f"b_{R.NAMES[t]}"]
    assert np.array_equal(R.dequantize(t, w, 128), Oracle().dequantize(t, w, 128))


# ---- the plan

KBLK_PLAN_PROBE = r"""
#include "qmm_kblk_plan.h"
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
static qmm_tensor dense(int type, int64_t ne0, int64_t ne1, int64_t ne2, uintptr_t data) {
    qmm_tensor t = {};
    t.type = type;  t.data = (void *) data;
    t.ne[0] = ne0;  t.ne[1] = ne1;  t.ne[2] = ne2;  t.ne[3] = 1;
    t.nb[0] = kblk_code(type) ? kblk_block(type) : type == G_F16 ? 2 : 4;
    t.nb[1] = kblk_code(type) ? ne0 / 32 * kblk_block(type) : t.nb[0] * ne0;
    t.nb[2] = t.nb[1] * ne1;  t.nb[3] = t.nb[2] * ne2;
    return t;
}
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {
        // decode type D Dv n_kv N H [SPLIT=0] | prefill type D n_kv N H Hk | cpy src_type dst_type ne0 ne1 ne2 dst_address | blocks
        std::istringstream in(spec);
        std::string family, kv;
        in >> family;
        if (family == "decode") {
            int type, D, Dv, n_kv, N, H;
            in >> type >> D >> Dv >> n_kv >> N >> H;
            AttnRules r = { true, true };
            while (in >> kv) { if (kv == "SPLIT=0") r.split_on = false; else return 1; }
            const AttnPlan p = kblk_decode_plan(r, type, D, Dv, n_kv, N, H);
            printf("%s%s%s grid=%u,%u,%u block=%u lds=%zu attr=%d S=%d chunk=%d ws=%zu merge=%u,%u,%u\n", p.label, p.label2[0] ? ";" : "", p.label2,
                   p.grid[0], p.grid[1], p.grid[2], p.block, p.lds, (int) p.lds_attr, p.S, p.chunk, p.ws_bytes, p.grid2[0], p.grid2[1], p.block2);
        } else if (family == "prefill") {
            int type, D, n_kv, N, H, Hk;
            in >> type >> D >> n_kv >> N >> H >> Hk;
            const KblkPrefillPlan p = kblk_prefill_plan(type, D, n_kv, N, H, Hk);
            printf("%s grid=%u block=%u threads=%u vec=%d ws=%zu k_nb=%lld,%lld;%s grid=%u,%u,%u block=%u lds=%zu attr=%d\n", p.unpack.label, p.unpack.grid,
                   p.unpack.block, p.unpack.threads, (int) p.unpack.vec, p.ws_bytes, (long long) p.k_nb1, (long long) p.k_nb2, p.attn.label, p.attn.grid[0],
                   p.attn.grid[1], p.attn.grid[2], p.attn.block, p.attn.lds, (int) p.attn.lds_attr);
        } else if (family == "cpy") {
            int ts, td;
            long long ne0, ne1, ne2, addr;
            in >> ts >> td >> ne0 >> ne1 >> ne2 >> addr;
            const qmm_tensor a = dense(ts, ne0, ne1, ne2, 1 << 20), d = dense(td, ne0, ne1, ne2, (uintptr_t) addr);
            const KblkCpyPlan p = kblk_cpy_plan(&a, &d);
            printf("sup=%d %s grid=%u block=%u threads=%u vec=%d\n", (int) kblk_takes_cpy(&a, &d), p.label, p.grid, p.block, p.threads, (int) p.vec);
        } else if (family == "blocks") {
            printf("%d %d %d %d\n", kblk_block(G_Q4_0), kblk_block(G_Q4_1), kblk_block(G_Q5_0), kblk_block(G_Q5_1));
        } else return 1;
    }
    return 0;
}
"""


def plan_table():
    """One line per decision, worked out by hand from the kernels' design, never printed by the header.  Few tokens: the Q8_0 form's launch
    under this kernel's label: one workgroup of 1024 threads per (head, token), 4 bytes of dynamic LDS per score of a piece; from 1024 cache
    rows on S = min(n_kv / 256, 16) pieces of ceil(n_kv / S) rounded up to 8 rows, a workspace of H * N * S * (Dv + 2) floats and the merge
    launch (H, N) x 256; SPLIT=0 keeps one piece.  Prompt: the unpack launch takes 8 values per thread of the D * n_kv * Hk it writes as f16
    into the workspace, then attn_prefill_kernel's own plan.  CPY: one thread per block into the type, 8 values per thread out of it."""
    rows = [("blocks", "18 20 22 24")]
    for t in R.TYPES:
        n = R.NAMES[t]
        rows += [
            (f"decode {t} 64 64 32 1 8", f"attn_kblk_decode_kernel<{n},64> grid=8,1,1 block=1024 lds=128 attr=0 S=0 chunk=32 ws=0 merge=0,0,0"),
            (f"decode {t} 128 128 992 2 8", f"attn_kblk_decode_kernel<{n},128> grid=8,2,1 block=1024 lds=3968 attr=0 S=0 chunk=992 ws=0 merge=0,0,0"),
            (f"decode {t} 128 128 1024 8 8", f"attn_kblk_decode_kernel<{n},128>;attn_combine_kernel grid=8,8,4 block=1024 lds=1024 attr=0 S=4 chunk=256 ws=133120 merge=8,8,256"),
            (f"decode {t} 64 64 1056 1 8", f"attn_kblk_decode_kernel<{n},64>;attn_combine_kernel grid=8,1,4 block=1024 lds=1056 attr=0 S=4 chunk=264 ws=8448 merge=8,1,256"),
            (f"decode {t} 128 128 16384 1 32", f"attn_kblk_decode_kernel<{n},128>;attn_combine_kernel grid=32,1,16 block=1024 lds=4096 attr=0 S=16 chunk=1024 ws=266240 merge=32,1,256"),
            (f"decode {t} 128 128 16384 1 8 SPLIT=0", f"attn_kblk_decode_kernel<{n},128> grid=8,1,1 block=1024 lds=65536 attr=1 S=0 chunk=16384 ws=0 merge=0,0,0"),
            (f"prefill {t} 64 64 33 8 2", f"cpy_{n}_unpack_kernel<f16> grid=4 block=256 threads=1024 vec=1 ws=16384 k_nb=128,8192;attn_prefill_kernel<64> grid=1,8,1 block=256 lds=35840 attr=0"),
            (f"prefill {t} 128 1056 130 8 2",
             f"cpy_{n}_unpack_kernel<f16> grid=132 block=256 threads=33792 vec=1 ws=540672 k_nb=256,270336;attn_prefill_kernel<128> grid=3,8,1 block=256 lds=150528 attr=1"),
            (f"cpy 0 {t} 128 8 4 1048576", f"sup=1 cpy_{n}_quantize_kernel grid=1 block=256 threads=128 vec=0"),
            (f"cpy 0 {t} 128 64 8 1048578", f"sup=1 cpy_{n}_quantize_kernel grid=8 block=256 threads=2048 vec=0"),
            (f"cpy {t} 0 64 3 1 1048576", f"sup=1 cpy_{n}_unpack_kernel<f32> grid=1 block=256 threads=24 vec=1"),
            (f"cpy {t} 1 128 2 5 1048584", f"sup=1 cpy_{n}_unpack_kernel<f16> grid=1 block=256 threads=160 vec=0"),
        ]
    return rows


@pytest.fixture(scope="module")
def kblk_plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each line of its input"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("kblkplan")
    (d / "probe.cpp").write_text(KBLK_PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_kblk_plan_keeps_every_decision(kblk_plan_probe):
    table = plan_table()
    got = kblk_plan_probe([spec for spec, _ in table])
    assert len(got) == len(table)
    for (spec, want), line in zip(table, got):
        assert line == want, spec


# ---- the predicates, through the library

@pytest.fixture(scope="module")
def lib():
    from ggml_hexagon_amd import build, capi
    lib = ctypes.CDLL(str(build.build_qmm()))
    P = ctypes.POINTER(capi.QmmTensor)
    lib.qmm_op_supported.argtypes = [ctypes.c_int, P, P, P, P]
    lib.qmm_attn_decode_supported.argtypes = [P, P, P, P, P]
    lib.qmm_attn_prefill_supported.argtypes = [P, P, P, P, P]
    lib.qmm_rope_kv_store_supported.argtypes = [P] * 8
    lib.qmm_attn_decode_rope_supported.argtypes = [P] * 12 + [ctypes.c_int64]
    return lib


F32, F16, Q8_0, Q4_K, I32 = 0, 1, 8, 12, 26
H, HK = 8, 2


def cpy(lib, a, d):
    from ggml_hexagon_amd import capi
    return lib.qmm_op_supported(capi.OP_CPY, ctypes.byref(a), None, None, ctypes.byref(d))


@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_cpy_into_and_out_of_the_type(lib, t):
    from ggml_hexagon_amd.capi import QmmTensor as T
    kb, B = (lambda *a, **k: R.kblk_tensor(t, *a, **k)), R.BLOCK[t]
    x = T.make(F32, [128, 8, 4])
    assert cpy(lib, x, kb([4096])) == 1                                                 # k_cur [D, H_kv, N] into the cache's 1-D view
    assert cpy(lib, x, kb([128, 8, 4])) == 1
    assert cpy(lib, T.make(F32, [128, 4, 8], nb=[4, 4096, 512, 16384]), kb([4096])) == 1          # any 4-byte strides of dims 1-3
    assert cpy(lib, T.make(F32, [48, 8, 4]), kb([1536])) == 0                           # rows of one and a half blocks
    assert cpy(lib, T.make(F32, [16, 8, 4]), kb([512])) == 0                            # rows of half a block
    assert cpy(lib, T.make(F32, [128, 8, 4], nb=[8, 1024, 8192, 32768]), kb([4096])) == 0         # src not dense along a row
    assert cpy(lib, T.make(F32, [128, 8, 4], nb=[4, 514, 4112, 16448]), kb([4096])) == 0          # src rows off 4 bytes
    assert cpy(lib, x, kb([128, 8, 4], nb=[B, 8 * B, 64 * B])) == 0                     # dst rows apart: not contiguous
    assert cpy(lib, x, kb([128, 8, 4], nb=[B + 2, 4 * (B + 2), 32 * (B + 2)])) == 0     # dst blocks not dense
    assert cpy(lib, x, kb([2048])) == 0                                                 # element counts differ
    assert cpy(lib, T.make(F16, [128, 8, 4]), kb([4096])) == 0                          # an f16 source is not built
    for dt in (F32, F16):
        assert cpy(lib, kb([128, 64, 2]), T.make(dt, [128, 64, 2])) == 1
        assert cpy(lib, kb([128, 64, 2], nb=[B, 8 * B, 4 * B]), T.make(dt, [128, 64, 2])) == 1     # the cache view llama.cpp makes: heads inside a row
        assert cpy(lib, kb([128, 64, 2], nb=[B, 8 * B + 1, 4 * B]), T.make(dt, [128, 64, 2])) == 0 # odd row stride
        assert cpy(lib, kb([128, 64, 2], nb=[2 * B, 8 * B, 4 * B]), T.make(dt, [128, 64, 2])) == 0 # blocks not dense
        assert cpy(lib, kb([128, 64, 2]), T.make(dt, [128, 64, 2], nb=[8, 1024, 65536, 131072])) == 0          # dst not contiguous
    assert cpy(lib, kb([128, 64, 2]), kb([128, 64, 2])) == 0 and cpy(lib, kb([128, 64]), T.make(I32, [128, 64])) == 0
    other = R.kblk_tensor([u for u in R.TYPES if u != t][0], [128, 64, 2])
    assert cpy(lib, kb([128, 64, 2]), other) == 0 and cpy(lib, kb([128, 64, 2]), T.make(Q8_0, [128, 64, 2], nb=[34, 136, 8704, 17408])) == 0
    assert cpy(lib, x, T.make(Q4_K, [128, 8, 4])) == 0                                  # the other quantized types stay refused
    assert cpy(lib, T.make(F32, [4096, 512]), T.make(F16, [4096, 512])) == 1            # the f32 / f16 surface is as it was


def kblk_operands(t, d, n_tok, n_kv, dv=None, h=H, hk=HK, n_ctx=None, mask_type=F32, k_nb=None, v_flags=0, v_type=F16):
    """llama.cpp's operands on a K cache of block type t and a transposed F16 V cache: k the permuted view of [n_embd_k_gqa, n_ctx] rows"""
    from ggml_hexagon_amd.capi import QmmTensor as T
    dv = dv or d
    n_ctx = n_ctx or n_kv + 64
    hb = R.BLOCK[t] * d // 32
    return [T.make(F32, [d, n_tok, h], nb=[4, h * d * 4, d * 4, n_tok * h * d * 4], data=1 << 20),
            R.kblk_tensor(t, [d, n_kv, hk], nb=k_nb or [R.BLOCK[t], hk * hb, hb], data=2 << 20),
            T.make(v_type, [n_kv, dv, hk], nb=[2, n_ctx * 2, n_ctx * dv * 2, n_ctx * dv * hk * 2], data=3 << 20, flags=v_flags),
            T.make(mask_type, [n_kv, 64 * ((n_tok + 63) // 64)], data=4 << 20), T.make(F32, [dv * h, n_tok], data=5 << 20)]


def ask(fn, ts):
    return fn(*[ctypes.byref(x) for x in ts])


@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_attention_takes_a_k_of_the_type_with_llama_cpp_strides(lib, t):
    dec, pre = lib.qmm_attn_decode_supported, lib.qmm_attn_prefill_supported
    ops = lambda *a, **k: kblk_operands(t, *a, **k)
    B = R.BLOCK[t]
    for d in (64, 128):
        assert ask(dec, ops(d, 1, 32)) == 1 and ask(dec, ops(d, 8, 16384)) == 1
        assert ask(pre, ops(d, 33, 64)) == 1 and ask(pre, ops(d, 512, 4096)) == 1 and ask(pre, ops(d, 1, 32)) == 1
    assert ask(dec, ops(128, 2, 96, dv=64)) == 1 and ask(dec, ops(64, 2, 96, dv=128)) == 1       # V rows of another width, few tokens only
    assert ask(dec, ops(128, 2, 96, hk=8)) == 1 and ask(dec, ops(128, 2, 96, h=32, hk=8)) == 1
    assert ask(dec, ops(128, 2, 96, k_nb=[B, 4 * B, 4 * B * 96])) == 1                           # contiguous [D, n_kv, H_kv]


@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_attention_limits_with_a_k_of_the_type(lib, t):
    dec, pre = lib.qmm_attn_decode_supported, lib.qmm_attn_prefill_supported
    ops = lambda *a, **k: kblk_operands(t, *a, **k)
    B = R.BLOCK[t]
    for fn, n in ((dec, 2), (pre, 70)):
        assert ask(fn, ops(128, n, 96)) == 1
        assert ask(fn, ops(256, n, 96)) == 0 and ask(fn, ops(96, n, 96)) == 0 and ask(fn, ops(32, n, 96)) == 0     # D in {64, 128}
        assert ask(fn, ops(128, n, 104)) == 0 and ask(fn, ops(128, n, 80)) == 0                     # n_kv in multiples of 32
        assert ask(fn, ops(128, n, 96, hk=3)) == 0                                                  # H no multiple of H_kv
        assert ask(fn, ops(128, n, 96, k_nb=[B, 8 * B + 1, 4 * B])) == 0 and ask(fn, ops(128, n, 96, k_nb=[B, 8 * B, 4 * B + 1])) == 0   # odd strides
        assert ask(fn, ops(128, n, 96, k_nb=[B + 2, 8 * B, 4 * B])) == 0                            # blocks not dense
        assert ask(fn, ops(128, n, 96, k_nb=[34, 8 * 34, 4 * 34])) == 0                             # ... nor Q8_0's block size
        assert ask(fn, ops(128, n, 96, mask_type=F16)) == 0                                         # the f16 mask comes with KV_ROWS only
        assert ask(fn, ops(128, n, 96, v_flags=1)) == 0 and ask(fn, ops(128, n, 96, v_flags=2)) == 0      # V stays the transposed cache
        assert ask(fn, ops(128, n, 96, v_type=Q8_0)) == 0 and ask(fn, ops(128, n, 96, v_type=t)) == 0     # ... in F16
        ts = ops(128, n, 96)
        ts[0].type = F16
        assert ask(fn, ts) == 0
    assert ask(dec, ops(128, 9, 96)) == 0 and ask(pre, ops(128, 9, 96)) == 1                        # 9 tokens: the prompt entry
    assert ask(dec, ops(128, 2, 96, dv=136)) == 0 and ask(dec, ops(128, 2, 96, dv=128)) == 1        # Dv <= 128
    assert ask(pre, ops(128, 70, 96, dv=64)) == 0                                                   # prompt: Dv == D
    assert ask(dec, ops(128, 2, 16384 + 32)) == 0 and ask(pre, ops(128, 2, 16384 + 32)) == 1        # past the few-token limit
    # the scratch cap of the prompt form: 64 MiB of f16 image = 131072 rows of 2 heads of 128
    assert ask(pre, ops(128, 70, 131072)) == 1 and ask(pre, ops(128, 70, 131072 + 32)) == 0
    assert ask(pre, ops(128, 70, 32768, h=32, hk=8)) == 1 and ask(pre, ops(128, 70, 32768 + 32, h=32, hk=8)) == 0
    ts = ops(128, 70, 96)
    ts[0].nb[1] += 8                                                                                # q rows off 16 bytes (float4 loads)
    assert ask(pre, ts) == 0


def f2i(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_rope_forms_refuse_the_type_and_still_take_f16(lib, t):
    """qmm_rope_kv_store refuses a k_dst of the type (the plugin stores through rope + CPY), and the one-launch rope + store + attention
    answers 0 for such a k_store / k whatever the other operands are; the same operands on an F16 cache are taken"""
    from ggml_hexagon_amd.capi import QmmTensor as T
    d, n, j0, n_kv, n_ctx = 128, 2, 37, 64, 256
    hb = R.BLOCK[t] * d // 32
    rope = [0, d, 0, 0, 8192, f2i(10000.0), f2i(1.0), f2i(0.0), f2i(1.0), f2i(32.0), f2i(1.0)]
    q = T.make(F32, [d, H, n], data=1 << 20)
    qd = T.make(F32, [d, H, n], data=2 << 20, op_params=rope)
    pos = T.make(I32, [n], data=3 << 20)
    k_new = T.make(F32, [d, HK, n], data=4 << 20)
    v_new = T.make(F32, [n, d * HK], nb=[d * HK * 4, 4, n * d * HK * 4, n * d * HK * 4], data=5 << 20)
    v_store = T.make(F16, [n, d * HK], nb=[2, n_ctx * 2, n_ctx * d * HK * 2, n_ctx * d * HK * 2], data=(6 << 20) + j0 * 2)
    v = T.make(F16, [n_kv, d, HK], nb=[2, n_ctx * 2, n_ctx * d * 2, n_ctx * d * HK * 2], data=6 << 20)
    mask = T.make(F32, [n_kv, 64], data=7 << 20)
    dst = T.make(F32, [d * H, n], data=8 << 20)
    k16 = T.make(F16, [d, n_kv, HK], nb=[2, HK * d * 2, d * 2, n_ctx * HK * d * 2], data=9 << 20)
    ks16 = T.make(F16, [d, HK, n], data=(9 << 20) + j0 * HK * d * 2)
    kq = R.kblk_tensor(t, [d, n_kv, HK], nb=[R.BLOCK[t], HK * hb, hb], data=9 << 20)
    ksq = R.kblk_tensor(t, [d, HK, n], data=(9 << 20) + j0 * HK * hb)
    r = ctypes.byref
    assert lib.qmm_rope_kv_store_supported(r(q), r(pos), None, r(qd), r(k_new), r(ks16), None, None) == 1
    assert lib.qmm_rope_kv_store_supported(r(q), r(pos), None, r(qd), r(k_new), r(ksq), None, None) == 0
    both = lambda ks, k: lib.qmm_attn_decode_rope_supported(r(q), r(pos), None, r(qd), r(k_new), r(ks), r(v_new), r(v_store), r(k), r(v), r(mask), r(dst), j0)
    assert both(ks16, k16) == 1
    assert both(ksq, kq) == 0 and both(ks16, kq) == 0 and both(ksq, k16) == 0
