"""CPU-side tests of the Q8_0 K cache (llama.cpp's -ctk q8_0 without flash attention; csrc/qmm_kcache_plan.h, csrc/qmm_kcache.hiph): the
launch plans through a probe the host compiler builds from the plan header alone, and what the entry points of include/ggml_mi355x_ops.h
take with a Q8_0 tensor among their operands through the library loaded without a device."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_kcache_plan.h"

KQ8_PLAN_PROBE = r"""
#include "qmm_kcache_plan.h"
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
static qmm_tensor dense(int type, int64_t ne0, int64_t ne1, int64_t ne2, uintptr_t data) {
    qmm_tensor t = {};
    t.type = type;  t.data = (void *) data;
    t.ne[0] = ne0;  t.ne[1] = ne1;  t.ne[2] = ne2;  t.ne[3] = 1;
    t.nb[0] = type == G_Q8_0 ? 34 : type == G_F16 ? 2 : 4;
    t.nb[1] = type == G_Q8_0 ? ne0 / 32 * 34 : t.nb[0] * ne0;
    t.nb[2] = t.nb[1] * ne1;  t.nb[3] = t.nb[2] * ne2;
    return t;
}
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {
        // decode D Dv n_kv N H [SPLIT=0] | prefill D n_kv N H Hk | cpy src_type dst_type ne0 ne1 ne2 dst_address | cap
        std::istringstream in(spec);
        std::string family, kv;
        in >> family;
        if (family == "decode") {
            int D, Dv, n_kv, N, H;
            in >> D >> Dv >> n_kv >> N >> H;
            AttnRules r = { true, true };
            while (in >> kv) { if (kv == "SPLIT=0") r.split_on = false; else return 1; }
            const AttnPlan p = kq8_decode_plan(r, D, Dv, n_kv, N, H);
            printf("%s%s%s grid=%u,%u,%u block=%u lds=%zu attr=%d S=%d chunk=%d ws=%zu merge=%u,%u,%u\n", p.label, p.label2[0] ? ";" : "", p.label2,
                   p.grid[0], p.grid[1], p.grid[2], p.block, p.lds, (int) p.lds_attr, p.S, p.chunk, p.ws_bytes, p.grid2[0], p.grid2[1], p.block2);
        } else if (family == "prefill") {
            int D, n_kv, N, H, Hk;
            in >> D >> n_kv >> N >> H >> Hk;
            const Kq8PrefillPlan p = kq8_prefill_plan(D, n_kv, N, H, Hk);
            printf("%s grid=%u block=%u threads=%u vec=%d ws=%zu k_nb=%lld,%lld;%s grid=%u,%u,%u block=%u lds=%zu attr=%d\n", p.unpack.label, p.unpack.grid,
                   p.unpack.block, p.unpack.threads, (int) p.unpack.vec, p.ws_bytes, (long long) p.k_nb1, (long long) p.k_nb2, p.attn.label, p.attn.grid[0],
                   p.attn.grid[1], p.attn.grid[2], p.attn.block, p.attn.lds, (int) p.attn.lds_attr);
        } else if (family == "cpy") {
            int ts, td;
            long long ne0, ne1, ne2, addr;
            in >> ts >> td >> ne0 >> ne1 >> ne2 >> addr;
            const qmm_tensor a = dense(ts, ne0, ne1, ne2, 1 << 20), d = dense(td, ne0, ne1, ne2, (uintptr_t) addr);
            const Kq8CpyPlan p = kq8_cpy_plan(&a, &d);
            printf("sup=%d %s grid=%u block=%u threads=%u vec=%d\n", (int) kq8_takes_cpy(&a, &d), p.label, p.grid, p.block, p.threads, (int) p.vec);
        } else if (family == "cap") {
            printf("cap=%zu static=%zu\n", KQ8_UNPACK_CAP, KQ8_STATIC_LDS);
        } else return 1;
    }
    return 0;
}
"""
# One line per decision, worked out by hand from the kernels' design, never printed by the header:
#   few tokens: one workgroup of 1024 threads per (head, token); dynamic LDS = 4 bytes per score of a piece; from 1024 cache rows on
#   S = min(n_kv / 256, 16) pieces of ceil(n_kv / S) rounded up to 8 rows, a workspace of H * N * S * (Dv + 2) floats and the merge launch
#   (H, N) x 256; SPLIT=0 keeps one piece, and at 16384 rows its 64 KiB of scores plus the static words need the raised LDS limit;
#   prompt: the unpack launch takes 8 values per thread of the D * n_kv * Hk it writes as f16 into the workspace (rows of D halves), then
#   attn_prefill_kernel's own plan (64 tokens per workgroup, 64 score rows of (min(n_kv, 512) + 4) floats + a tile of 128 x 72 halves);
#   CPY: 4 values per thread into Q8_0, 8 per thread out of it, 16-byte stores where the destination allows them.
KQ8_PLAN_TABLE = [
    ("decode 64 64 32 1 8", "attn_kq8_decode_kernel<64> grid=8,1,1 block=1024 lds=128 attr=0 S=0 chunk=32 ws=0 merge=0,0,0"),
    ("decode 128 128 992 2 8", "attn_kq8_decode_kernel<128> grid=8,2,1 block=1024 lds=3968 attr=0 S=0 chunk=992 ws=0 merge=0,0,0"),
    ("decode 128 128 1024 8 8", "attn_kq8_decode_kernel<128>;attn_combine_kernel grid=8,8,4 block=1024 lds=1024 attr=0 S=4 chunk=256 ws=133120 merge=8,8,256"),
    ("decode 64 64 1056 1 8", "attn_kq8_decode_kernel<64>;attn_combine_kernel grid=8,1,4 block=1024 lds=1056 attr=0 S=4 chunk=264 ws=8448 merge=8,1,256"),
    ("decode 128 128 4160 2 8", "attn_kq8_decode_kernel<128>;attn_combine_kernel grid=8,2,16 block=1024 lds=1056 attr=0 S=16 chunk=264 ws=133120 merge=8,2,256"),
    ("decode 128 128 16384 1 32", "attn_kq8_decode_kernel<128>;attn_combine_kernel grid=32,1,16 block=1024 lds=4096 attr=0 S=16 chunk=1024 ws=266240 merge=32,1,256"),
    ("decode 128 64 1024 1 8", "attn_kq8_decode_kernel<128>;attn_combine_kernel grid=8,1,4 block=1024 lds=1024 attr=0 S=4 chunk=256 ws=8448 merge=8,1,256"),
    ("decode 128 128 4096 1 8 SPLIT=0", "attn_kq8_decode_kernel<128> grid=8,1,1 block=1024 lds=16384 attr=0 S=0 chunk=4096 ws=0 merge=0,0,0"),
    ("decode 128 128 16384 1 8 SPLIT=0", "attn_kq8_decode_kernel<128> grid=8,1,1 block=1024 lds=65536 attr=1 S=0 chunk=16384 ws=0 merge=0,0,0"),
    ("prefill 64 64 33 8 2", "cpy_q8_0_unpack_kernel<f16> grid=4 block=256 threads=1024 vec=1 ws=16384 k_nb=128,8192;attn_prefill_kernel<64> grid=1,8,1 block=256 lds=35840 attr=0"),
    ("prefill 128 1056 130 8 2",
     "cpy_q8_0_unpack_kernel<f16> grid=132 block=256 threads=33792 vec=1 ws=540672 k_nb=256,270336;attn_prefill_kernel<128> grid=3,8,1 block=256 lds=150528 attr=1"),
    ("cpy 0 8 128 8 4 1048576", "sup=1 cpy_q8_0_quantize_kernel grid=4 block=256 threads=1024 vec=0"),
    ("cpy 0 8 64 3 1 1048578", "sup=1 cpy_q8_0_quantize_kernel grid=1 block=256 threads=48 vec=0"),
    ("cpy 8 0 64 3 1 1048576", "sup=1 cpy_q8_0_unpack_kernel<f32> grid=1 block=256 threads=24 vec=1"),
    ("cpy 8 1 128 2 5 1048584", "sup=1 cpy_q8_0_unpack_kernel<f16> grid=1 block=256 threads=160 vec=0"),
    ("cap", "cap=67108864 static=256"),
]


@pytest.fixture(scope="module")
def kq8_plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each line of its input"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("kq8plan")
    (d / "probe.cpp").write_text(KQ8_PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_kq8_plan_keeps_every_decision(kq8_plan_probe):
    got = kq8_plan_probe([spec for spec, _ in KQ8_PLAN_TABLE])
    assert len(got) == len(KQ8_PLAN_TABLE)
    for (spec, want), line in zip(KQ8_PLAN_TABLE, got):
        assert line == want, spec


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


F32, F16, Q8_0, Q4_K, BF16, I32 = 0, 1, 8, 12, 30, 26
H, HK = 8, 2


def q8(ne, nb=None, data=1 << 20):
    """a Q8_0 descriptor: contiguous rows of 34-byte blocks unless byte strides are given"""
    from ggml_hexagon_amd.capi import QmmTensor as T
    ne = list(ne) + [1] * (4 - len(ne))
    if nb is None:
        nb, acc = [34], ne[0] // 32 * 34
        for n in ne[1:]:
            nb.append(acc)
            acc *= n
    return T.make(Q8_0, ne, nb=list(nb) + [nb[-1] * ne[len(nb) - 1]] * (4 - len(nb)), data=data)


def cpy(lib, a, d):
    from ggml_hexagon_amd import capi
    return lib.qmm_op_supported(capi.OP_CPY, ctypes.byref(a), None, None, ctypes.byref(d))


def test_cpy_into_and_out_of_q8_0(lib):
    from ggml_hexagon_amd.capi import QmmTensor as T
    x = T.make(F32, [128, 8, 4])
    assert cpy(lib, x, q8([4096])) == 1                                                 # k_cur [D, H_kv, N] into the cache's 1-D view
    assert cpy(lib, x, q8([128, 8, 4])) == 1
    assert cpy(lib, T.make(F32, [128, 4, 8], nb=[4, 4096, 512, 16384]), q8([4096])) == 1          # any 4-byte strides of dims 1-3
    assert cpy(lib, T.make(F32, [48, 8, 4]), q8([1536])) == 0                           # rows of one and a half blocks
    assert cpy(lib, T.make(F32, [128, 8, 4], nb=[8, 1024, 8192, 32768]), q8([4096])) == 0         # src not dense along a row
    assert cpy(lib, T.make(F32, [128, 8, 4], nb=[4, 514, 4112, 16448]), q8([4096])) == 0          # src rows off 4 bytes
    assert cpy(lib, x, q8([128, 8, 4], nb=[34, 272, 2176])) == 0                        # dst rows apart: not contiguous
    assert cpy(lib, x, q8([2048])) == 0                                                 # element counts differ
    assert cpy(lib, T.make(F16, [128, 8, 4]), q8([4096])) == 0                          # f16 -> Q8_0 is not built
    assert cpy(lib, x, T.make(Q4_K, [128, 8, 4])) == 0 and cpy(lib, x, T.make(BF16, [128, 8, 4])) == 0
    assert cpy(lib, T.make(F32, [4096, 512]), T.make(Q4_K, [4096, 512])) == 0 and cpy(lib, T.make(F32, [4096, 512]), T.make(BF16, [4096, 512])) == 0
    for t in (F32, F16):
        assert cpy(lib, q8([128, 64, 2]), T.make(t, [128, 64, 2])) == 1
        assert cpy(lib, q8([128, 64, 2], nb=[34, 272, 136]), T.make(t, [128, 64, 2])) == 1         # the cache view llama.cpp makes: heads inside a row
        assert cpy(lib, q8([128, 64, 2], nb=[34, 273, 136]), T.make(t, [128, 64, 2])) == 0         # odd row stride
        assert cpy(lib, q8([128, 64, 2], nb=[68, 272, 136]), T.make(t, [128, 64, 2])) == 0         # blocks not dense
        assert cpy(lib, q8([128, 64, 2]), T.make(t, [128, 64, 2], nb=[8, 1024, 65536, 131072])) == 0          # dst not contiguous
    assert cpy(lib, q8([128, 64, 2]), q8([128, 64, 2])) == 0 and cpy(lib, q8([128, 64]), T.make(I32, [128, 64])) == 0
    assert cpy(lib, T.make(F32, [4096, 512]), T.make(F16, [4096, 512])) == 1            # the f32 / f16 surface is as it was


def kq8_operands(d, n_tok, n_kv, dv=None, h=H, hk=HK, n_ctx=None, mask_type=F32, k_nb=None, v_flags=0, v_type=F16):
    """llama.cpp's operands on a Q8_0 K cache and a transposed F16 V cache: k the permuted view of [n_embd_k_gqa, n_ctx] rows"""
    from ggml_hexagon_amd.capi import QmmTensor as T
    dv = dv or d
    n_ctx = n_ctx or n_kv + 64
    hb = 34 * d // 32
    return (T.make(F32, [d, n_tok, h], nb=[4, h * d * 4, d * 4, n_tok * h * d * 4], data=1 << 20),
            q8([d, n_kv, hk], nb=k_nb or [34, hk * hb, hb], data=2 << 20),
            T.make(v_type, [n_kv, dv, hk], nb=[2, n_ctx * 2, n_ctx * dv * 2, n_ctx * dv * hk * 2], data=3 << 20, flags=v_flags),
            T.make(mask_type, [n_kv, 64 * ((n_tok + 63) // 64)], data=4 << 20), T.make(F32, [dv * h, n_tok], data=5 << 20))


def ask(fn, ts):
    return fn(*[ctypes.byref(t) for t in ts])


def test_attention_takes_a_q8_0_k_with_llama_cpp_strides(lib):
    dec, pre = lib.qmm_attn_decode_supported, lib.qmm_attn_prefill_supported
    for d in (64, 128):
        assert ask(dec, kq8_operands(d, 1, 32)) == 1 and ask(dec, kq8_operands(d, 8, 16384)) == 1
        assert ask(pre, kq8_operands(d, 33, 64)) == 1 and ask(pre, kq8_operands(d, 512, 4096)) == 1 and ask(pre, kq8_operands(d, 1, 32)) == 1
    assert ask(dec, kq8_operands(128, 2, 96, dv=64)) == 1 and ask(dec, kq8_operands(64, 2, 96, dv=128)) == 1       # V rows of another width, few tokens only
    assert ask(dec, kq8_operands(128, 2, 96, hk=8)) == 1 and ask(dec, kq8_operands(128, 2, 96, h=32, hk=8)) == 1
    assert ask(dec, kq8_operands(128, 2, 96, k_nb=[34, 136, 136 * 96])) == 1                                          # contiguous [D, n_kv, H_kv]


def test_attention_limits_with_a_q8_0_k(lib):
    dec, pre = lib.qmm_attn_decode_supported, lib.qmm_attn_prefill_supported
    for fn, n in ((dec, 2), (pre, 70)):
        assert ask(fn, kq8_operands(128, n, 96)) == 1
        assert ask(fn, kq8_operands(256, n, 96)) == 0 and ask(fn, kq8_operands(96, n, 96)) == 0 and ask(fn, kq8_operands(32, n, 96)) == 0     # D in {64, 128}
        assert ask(fn, kq8_operands(128, n, 104)) == 0 and ask(fn, kq8_operands(128, n, 80)) == 0                     # n_kv in multiples of 32
        assert ask(fn, kq8_operands(128, n, 96, hk=3)) == 0                                                           # H no multiple of H_kv
        assert ask(fn, kq8_operands(128, n, 96, k_nb=[34, 273, 136])) == 0 and ask(fn, kq8_operands(128, n, 96, k_nb=[34, 272, 137])) == 0   # odd strides
        assert ask(fn, kq8_operands(128, n, 96, k_nb=[36, 272, 136])) == 0                                            # blocks not dense
        assert ask(fn, kq8_operands(128, n, 96, mask_type=F16)) == 0                                                  # the f16 mask comes with KV_ROWS only
        assert ask(fn, kq8_operands(128, n, 96, v_flags=1)) == 0 and ask(fn, kq8_operands(128, n, 96, v_flags=2)) == 0      # V stays the transposed cache
        assert ask(fn, kq8_operands(128, n, 96, v_type=Q8_0)) == 0                                                    # ... in F16
        ts = kq8_operands(128, n, 96)
        ts[0].type = F16
        assert ask(fn, ts) == 0
    assert ask(dec, kq8_operands(128, 9, 96)) == 0 and ask(pre, kq8_operands(128, 9, 96)) == 1                        # 9 tokens: the prompt entry
    assert ask(dec, kq8_operands(128, 2, 96, dv=136)) == 0 and ask(dec, kq8_operands(128, 2, 96, dv=128)) == 1        # Dv <= 128
    assert ask(pre, kq8_operands(128, 70, 96, dv=64)) == 0                                                            # prompt: Dv == D
    assert ask(dec, kq8_operands(128, 2, 16384 + 32)) == 0 and ask(pre, kq8_operands(128, 2, 16384 + 32)) == 1        # past the few-token limit
    # the scratch cap of the prompt form: 64 MiB of f16 image = 131072 rows of 2 heads of 128
    assert ask(pre, kq8_operands(128, 70, 131072)) == 1 and ask(pre, kq8_operands(128, 70, 131072 + 32)) == 0
    assert ask(pre, kq8_operands(128, 70, 32768, h=32, hk=8)) == 1 and ask(pre, kq8_operands(128, 70, 32768 + 32, h=32, hk=8)) == 0
    ts = kq8_operands(128, 70, 96)
    ts[0].nb[1] += 8                                                                                                  # q rows off 16 bytes (float4 loads)
    assert ask(pre, ts) == 0


def test_rope_forms_stay_f16_only(lib):
    """qmm_rope_kv_store keeps refusing a Q8_0 k_dst (the plugin stores through rope + CPY), and the one-launch rope + store + attention
    answers 0 for a Q8_0 k_store / k whatever the other operands are; the same operands on an F16 cache are taken"""
    from ggml_hexagon_amd.capi import QmmTensor as T
    d, n, j0, n_kv, n_ctx = 128, 2, 37, 64, 256
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
    k8 = q8([d, n_kv, HK], nb=[34, HK * 136, 136], data=9 << 20)
    ks8 = q8([d, HK, n], data=(9 << 20) + j0 * HK * 136)
    r = ctypes.byref
    assert lib.qmm_rope_kv_store_supported(r(q), r(pos), None, r(qd), r(k_new), r(ks16), None, None) == 1
    assert lib.qmm_rope_kv_store_supported(r(q), r(pos), None, r(qd), r(k_new), r(ks8), None, None) == 0
    both = lambda ks, k: lib.qmm_attn_decode_rope_supported(r(q), r(pos), None, r(qd), r(k_new), r(ks), r(v_new), r(v_store), r(k), r(v), r(mask), r(dst), j0)
    assert both(ks16, k16) == 1
    assert both(ks8, k8) == 0 and both(ks16, k8) == 0 and both(ks8, k16) == 0


def f2i(x):
    import struct
    return struct.unpack("<i", struct.pack("<f", x))[0]
