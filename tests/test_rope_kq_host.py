"""CPU-side tests of qmm_rope_kq_store (csrc/qmm_ropekq_plan.h, csrc/qmm_ropekq.hiph): rope(q), rope(k) into a K cache of Q8_0, Q4_0, Q4_1, Q5_0 or
Q5_1 blocks and the V store as one launch.  What the new predicate takes and refuses, asked through the library loaded without a device
with llama.cpp's operands; that the two older rope entry points keep refusing such a cache (and keep taking F16); and the launch plan
through a probe the host compiler builds from the plan header alone."""
import ctypes
import itertools
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_ropekq_plan.h"

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, IQ4_NL, I32 = 0, 1, 2, 3, 6, 7, 8, 12, 20, 26
BLOCK = {Q8_0: 34, Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24}
NAMES = {Q8_0: "q8_0", Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1"}
TYPES = list(BLOCK)
TYPE_IDS = [NAMES[t] for t in TYPES]


@pytest.fixture(scope="module")
def lib():
    from ggml_hexagon_amd import build, capi
    lib = ctypes.CDLL(str(build.build_qmm()))
    P = ctypes.POINTER(capi.QmmTensor)
    lib.qmm_rope_kq_store_supported.argtypes = [P] * 8           # (on a library without the entry point this is where the file fails)
    lib.qmm_rope_kv_store_supported.argtypes = [P] * 8
    lib.qmm_attn_decode_rope_supported.argtypes = [P] * 12 + [ctypes.c_int64]
    return lib


def f2i(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def blocks(t, ne, nb=None, data=9 << 20, block=None):
    """a descriptor of block type t (any type code: `block` bytes per 32 values): contiguous rows of blocks unless byte strides are given"""
    from ggml_hexagon_amd.capi import QmmTensor
    b = block or BLOCK[t]
    ne = list(ne) + [1] * (4 - len(ne))
    if nb is None:
        nb, acc = [b], ne[0] // 32 * b
        for n in ne[1:]:
            nb.append(acc)
            acc *= n
    return QmmTensor.make(t, ne, nb=list(nb), data=data)


def operands(t, d=128, h=8, hk=2, n=2, v=True, ff=False, mode=0, n_dims=None, j0=37, n_ctx=1024):
    """llama.cpp's operands of build_attn's rope and stores on a K cache of block type t and a transposed F16 V cache, by name"""
    from ggml_hexagon_amd.capi import QmmTensor as T
    rope = [0, n_dims or d, mode, 0, 8192, f2i(10000.0), f2i(1.0), f2i(0.0), f2i(1.0), f2i(32.0), f2i(1.0)]
    o = {"q": T.make(F32, [d, h, n], data=1 << 20), "pos": T.make(I32, [n], data=3 << 20), "ff": T.make(F32, [d // 2], data=10 << 20) if ff else None,
         "q_dst": T.make(F32, [d, h, n], data=2 << 20, op_params=rope), "k": T.make(F32, [d, hk, n], data=4 << 20),
         "k_dst": blocks(t, [d, hk, n], data=(9 << 20) + j0 * hk * d // 32 * BLOCK[t]), "v": None, "v_dst": None}
    if v:
        o["v"] = T.make(F32, [n, d * hk], nb=[d * hk * 4, 4, n * d * hk * 4, n * d * hk * 4], data=5 << 20)              # v_cur^T
        o["v_dst"] = T.make(F16, [n, d * hk], nb=[2, n_ctx * 2, n_ctx * d * hk * 2, n_ctx * d * hk * 2], data=(6 << 20) + j0 * 2)
    return o


ORDER = ("q", "pos", "ff", "q_dst", "k", "k_dst", "v", "v_dst")


def ask(fn, o, **swap):
    o = dict(o, **swap)
    return fn(*[ctypes.byref(o[name]) if o[name] is not None else None for name in ORDER])


@pytest.mark.parametrize("t", TYPES, ids=TYPE_IDS)
def test_predicate_takes_llama_cpp_operands(lib, t):
    sup = lib.qmm_rope_kq_store_supported
    count = 0
    for d, n, v, ff, mode in itertools.product((64, 128, 256), (1, 8, 512), (False, True), (False, True), (0, 2)):
        assert ask(sup, operands(t, d=d, n=n, v=v, ff=ff, mode=mode, j0=0)) == 1, (d, n, v, ff, mode)
        count += 1
    assert count == 72
    for d, mode in itertools.product((64, 128, 256), (0, 2)):
        assert ask(sup, operands(t, d=d, n_dims=d // 2, mode=mode)) == 1                    # partial rotation
    assert ask(sup, operands(t, h=32, hk=8, n=1)) == 1 and ask(sup, operands(t, h=64, hk=8, n=512, j0=0)) == 1       # llama3-8b's and 70b's heads
    assert ask(sup, operands(t, d=256, h=32, hk=32, n=70)) == 1                             # the largest staged token: 8192 values
    o = operands(t, n=4)
    from ggml_hexagon_amd.capi import QmmTensor as T
    assert ask(sup, o, k=T.make(F32, [128, 2, 4], nb=[4, 512, 4096, 16384], data=4 << 20)) == 1      # k a view: tokens further apart


@pytest.mark.parametrize("t", TYPES, ids=TYPE_IDS)
def test_predicate_refuses(lib, t):
    from ggml_hexagon_amd.capi import QmmTensor as T
    sup = lib.qmm_rope_kq_store_supported
    B, d, hk, n = BLOCK[t], 128, 2, 2
    o = operands(t)
    assert ask(sup, o) == 1
    assert ask(sup, o, k_dst=T.make(F16, [d, hk, n], data=9 << 20)) == 0                               # an F16 k_dst is qmm_rope_kv_store's
    assert ask(sup, o, k_dst=blocks(IQ4_NL, [d, hk, n], block=18)) == 0                                # IQ4_NL
    assert ask(sup, o, k_dst=blocks(Q4_K, [d, hk, n], block=18)) == 0 and ask(sup, o, k_dst=T.make(F32, [d, hk, n], data=9 << 20)) == 0   # every other type
    for dd in (48, 16):                                                                                # rows of partial blocks
        p = operands(t, d=dd)
        p["k_dst"] = blocks(t, [dd, hk, n], nb=[B, max(dd // 32, 1) * B, max(dd // 32, 1) * B * hk, max(dd // 32, 1) * B * hk * n])
        assert ask(sup, p) == 0
    assert ask(sup, o, k_dst=blocks(t, [d, hk, n], nb=[B, 8 * B, 16 * B, 32 * B])) == 0                # k_dst rows apart: not contiguous
    assert ask(sup, o, k_dst=blocks(t, [d, hk, n], nb=[B + 2, 4 * (B + 2), 8 * (B + 2), 16 * (B + 2)])) == 0        # blocks not dense
    for mode in (4, 8, 24, 1):                                                                         # a rope mode other than normal / NEOX
        assert ask(sup, operands(t, mode=mode)) == 0
    assert ask(sup, o, k=None) == 0 and ask(sup, o, k_dst=None) == 0 and ask(sup, o, k=None, k_dst=None) == 0        # the K pair is required
    assert ask(sup, o, k_dst=blocks(t, [d, hk, n + 1])) == 0 and ask(sup, o, k_dst=blocks(t, [d * hk * n])) == 0     # extents differ from k's
    assert ask(sup, o, k=T.make(F32, [d, hk, n], nb=[4, 514, 1028, 2056], data=4 << 20)) == 0          # k rows off 4 bytes
    assert ask(sup, o, k=T.make(F32, [d, hk, n], nb=[8, 1024, 2048, 4096], data=4 << 20)) == 0         # k not dense along a row
    assert ask(sup, o, k=T.make(F32, [d, hk, n], data=(4 << 20) + 2)) == 0                             # k data off 4 bytes
    assert ask(sup, o, k=T.make(F16, [d, hk, n], data=4 << 20)) == 0                                   # an f16 k
    assert ask(sup, o, k_dst=blocks(t, [d, hk, n], data=(9 << 20) + 1)) == 0                           # an odd k_dst data pointer
    assert ask(sup, operands(t, d=256, h=33, hk=33, n=2)) == 0                                         # one head past the staged token (8448 values)
    assert ask(sup, operands(t, d=32, h=257, hk=257, n=1)) == 0                                        # ... one block past it (8224)
    assert ask(sup, o, k=T.make(F32, [d, hk, n + 1], data=4 << 20), k_dst=blocks(t, [d, hk, n + 1])) == 0   # another token count than q's
    assert ask(sup, o, k=T.make(F32, [64, hk, n], data=4 << 20), k_dst=blocks(t, [64, hk, n])) == 0    # another head size than q's
    assert ask(sup, o, q=None) == 0 and ask(sup, o, pos=None) == 0 and ask(sup, o, q_dst=None) == 0
    assert ask(sup, o, v_dst=None) == 0                                                                # v without its destination
    assert ask(sup, o, v_dst=T.make(F32, [n, d * hk], data=6 << 20)) == 0                              # V stays F16
    assert ask(sup, operands(t, n_dims=d + 2)) == 0 and ask(sup, operands(t, n_dims=63)) == 0          # sup_rope's n_dims rules


@pytest.mark.parametrize("t", TYPES, ids=TYPE_IDS)
def test_the_older_rope_entry_points_keep_their_surface(lib, t):
    """the same quantized operands: qmm_rope_kv_store and qmm_attn_decode_rope answer 0, and 1 on an F16 cache"""
    from ggml_hexagon_amd.capi import QmmTensor as T
    d, h, hk, n, j0, n_kv, n_ctx = 128, 8, 2, 2, 37, 64, 1024
    o = operands(t, j0=j0, n_ctx=n_ctx)
    assert ask(lib.qmm_rope_kq_store_supported, o) == 1
    assert ask(lib.qmm_rope_kv_store_supported, o) == 0
    ks16 = T.make(F16, [d, hk, n], data=(9 << 20) + j0 * hk * d * 2)
    assert ask(lib.qmm_rope_kv_store_supported, o, k_dst=ks16) == 1 and ask(lib.qmm_rope_kq_store_supported, o, k_dst=ks16) == 0
    hb = BLOCK[t] * d // 32
    v = T.make(F16, [n_kv, d, hk], nb=[2, n_ctx * 2, n_ctx * d * 2, n_ctx * d * hk * 2], data=6 << 20)
    mask, dst = T.make(F32, [n_kv, 64], data=7 << 20), T.make(F32, [d * h, n], data=8 << 20)
    k16 = T.make(F16, [d, n_kv, hk], nb=[2, hk * d * 2, d * 2, n_ctx * hk * d * 2], data=9 << 20)
    kq = blocks(t, [d, n_kv, hk], nb=[BLOCK[t], hk * hb, hb, n_ctx * hk * hb], data=9 << 20)
    r = ctypes.byref
    both = lambda ks, k: lib.qmm_attn_decode_rope_supported(r(o["q"]), r(o["pos"]), None, r(o["q_dst"]), r(o["k"]), r(ks), r(o["v"]), r(o["v_dst"]), r(k), r(v),
                                                            r(mask), r(dst), j0)
    assert both(ks16, k16) == 1
    assert both(o["k_dst"], kq) == 0 and both(ks16, kq) == 0 and both(o["k_dst"], k16) == 0


# ---- the plan

ROPEKQ_PLAN_PROBE = r"""
#include "qmm_ropekq_plan.h"
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
static qmm_tensor dense(int type, int64_t ne0, int64_t ne1, int64_t ne2, uintptr_t data) {
    qmm_tensor t = {};
    t.type = type;  t.data = (void *) data;
    t.ne[0] = ne0;  t.ne[1] = ne1;  t.ne[2] = ne2;  t.ne[3] = 1;
    t.nb[0] = ropekq_code(type) ? ropekq_block(type) : type == G_F16 ? 2 : 4;
    t.nb[1] = ropekq_code(type) ? ne0 / 32 * ropekq_block(type) : t.nb[0] * ne0;
    t.nb[2] = t.nb[1] * ne1;  t.nb[3] = t.nb[2] * ne2;
    return t;
}
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {
        // type D H H_kv N v (0: no v pair, 1: v_cur^T into the transposed cache)
        std::istringstream in(spec);
        std::string family;
        in >> family;
        if (family == "limit") { printf("%lld %u\n", (long long) ROPEKQ_MAX_ROW, ROPEKQ_BLOCK); continue; }
        if (family != "store") return 1;
        int type, D, H, Hk, N, has_v;
        in >> type >> D >> H >> Hk >> N >> has_v;
        qmm_tensor q = dense(G_F32, D, H, N, 1 << 20), qd = q, pos = dense(G_I32, N, 1, 1, 3 << 20), k = dense(G_F32, D, Hk, N, 4 << 20), kd = dense(type, D, Hk, N, 9 << 20);
        qd.op_params[1] = D;
        qmm_tensor v = dense(G_F32, N, (int64_t) D * Hk, 1, 5 << 20), vd = dense(G_F16, N, (int64_t) D * Hk, 1, 6 << 20);
        v.nb[0] = (int64_t) D * Hk * 4;  v.nb[1] = 4;  vd.nb[1] = 2048;
        const bool sup = ropekq_takes_store(&q, &pos, nullptr, &qd, &k, &kd, has_v ? &v : nullptr, has_v ? &vd : nullptr);
        if (!sup) { printf("sup=0\n"); continue; }
        const RopeKqPlan p = rope_kq_store_plan(&q, &k, &kd, has_v ? &v : nullptr, has_v ? &vd : nullptr);
        printf("sup=1 %s grid=%u=%u+%u+%u block=%u lds=%zu tiles0=%u\n", p.label, p.grid, p.q_blocks, p.k_blocks, p.v_blocks, p.block, p.lds, p.tiles0);
    }
    return 0;
}
"""


def plan_table():
    """One line per decision, worked out by hand from the kernel's design, never printed by the header.  The grid is q's blocks (a thread per
    (pair, 8 heads, token): D / 2 * ceil(H / 8) * N threads in blocks of 256), one block per token of k, and v's blocks: 32 x 32 tiles where
    v^T has at least 32 tokens, otherwise an element per thread.  Dynamic LDS: the staged token, 4 * D * H_kv bytes, at most 32 KiB."""
    return [
        ("limit", "8192 256"),
        # llama3-8b, one token: q 64 * 4 = 256 threads; v 1024 elements
        (f"store {Q8_0} 128 32 8 1 1", "sup=1 rope_kq_store_kernel<q8_0,false> grid=6=1+1+4 block=256 lds=4096 tiles0=0"),
        # ... a prompt batch: q 64 * 4 * 512 threads; v 16 x 32 tiles
        (f"store {Q4_0} 128 32 8 512 1", "sup=1 rope_kq_store_kernel<q4_0,true> grid=1536=512+512+512 block=256 lds=4096 tiles0=16"),
        # the smallest launch: one block for q, one for k
        (f"store {Q5_1} 64 1 1 1 0", "sup=1 rope_kq_store_kernel<q5_1,false> grid=2=1+1+0 block=256 lds=256 tiles0=0"),
        # a short head chunk, q's threads and v's elements no multiple of 256: 320 and 1920
        (f"store {Q4_1} 128 6 3 5 1", "sup=1 rope_kq_store_kernel<q4_1,false> grid=15=2+5+8 block=256 lds=1536 tiles0=0"),
        # 31 tokens: still element-wise; 32: tiles
        (f"store {Q5_0} 128 8 2 31 1", "sup=1 rope_kq_store_kernel<q5_0,false> grid=70=8+31+31 block=256 lds=1024 tiles0=0"),
        (f"store {Q5_0} 128 8 2 32 1", "sup=1 rope_kq_store_kernel<q5_0,true> grid=48=8+32+8 block=256 lds=1024 tiles0=1"),
        (f"store {Q8_0} 128 8 2 70 1", "sup=1 rope_kq_store_kernel<q8_0,true> grid=112=18+70+24 block=256 lds=1024 tiles0=3"),
        # the largest token the staging admits (8192 values), and one head / one block past it
        (f"store {Q5_0} 256 32 32 70 1", "sup=1 rope_kq_store_kernel<q5_0,true> grid=978=140+70+768 block=256 lds=32768 tiles0=3"),
        (f"store {Q5_0} 256 33 33 70 1", "sup=0"),
        (f"store {Q8_0} 32 257 257 1 0", "sup=0"),
        (f"store {Q8_0} 32 256 256 1 0", "sup=1 rope_kq_store_kernel<q8_0,false> grid=3=2+1+0 block=256 lds=32768 tiles0=0"),
        (f"store {F16} 128 8 2 2 1", "sup=0"),
        (f"store {IQ4_NL} 128 8 2 2 1", "sup=0"),
    ]


@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each line of its input"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("ropekqplan")
    (d / "probe.cpp").write_text(ROPEKQ_PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_plan_keeps_every_decision(plan_probe):
    table = plan_table()
    got = plan_probe([spec for spec, _ in table])
    assert len(got) == len(table)
    for (spec, want), line in zip(table, got):
        assert line == want, spec
