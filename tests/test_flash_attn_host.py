"""CPU-side tests of GGML_OP_FLASH_ATTN_EXT's way through the attention ABI (include/ggml_mi355x_ops.h, QMM_TENSOR_KV_ROWS on the v
operand): the launch plans of the two kernels (csrc/qmm_attn_plan.h: attn_rows_decode_plan, attn_rows_prefill_plan) through a probe the
host compiler builds from the header alone, and the _supported predicates through the library loaded without a device."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ATTN_PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_attn_plan.h"

ROWS_PLAN_PROBE = r"""
#include "qmm_attn_plan.h"
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {          // decode D n_kv N H mask_f16 [SPLIT=0]  |  prefill D n_kv N H mask_f16
        std::istringstream in(spec);
        std::string family, kv;
        int D, n_kv, N, H, m16;
        in >> family >> D >> n_kv >> N >> H >> m16;
        AttnRules r = { true, true };
        while (in >> kv) { if (kv == "SPLIT=0") r.split_on = false; else return 1; }
        const AttnPlan p = family == "prefill" ? attn_rows_prefill_plan(D, n_kv, N, H, m16 != 0) : attn_rows_decode_plan(r, D, n_kv, N, H, m16 != 0);
        printf("%s%s%s grid=%u,%u,%u block=%u lds=%zu attr=%d S=%d chunk=%d ws=%zu merge=%u,%u,%u m16=%d rows=%d\n", p.label, p.label2[0] ? ";" : "", p.label2,
               p.grid[0], p.grid[1], p.grid[2], p.block, p.lds, (int) p.lds_attr, p.S, p.chunk, p.ws_bytes, p.grid2[0], p.grid2[1], p.block2, (int) p.mask_f16,
               (int) (p.kernel == AK_ROWS_DECODE || p.kernel == AK_ROWS_PREFILL));
    }
    return 0;
}
"""
# One line per branch, worked out by hand from the kernels' design, never printed by the header:
#   few tokens: LDS = 4 bytes per score of a piece + 16 waves x D f32 partial sums; from 1024 cache rows on S = min(n_kv / 256, 16) pieces of
#   ceil(n_kv / S) rounded up to 8 rows, a workspace of H * N * S * (D + 2) floats and the merge launch (H, N) x 256; SPLIT=0 keeps one piece;
#   prompt: 64 tokens per workgroup, LDS = 64 score rows of (min(n_kv, 512) + 4) floats + a tile of 128 x (64 + 8) halves; past 64 KiB the
#   kernel's limit has to be raised.
ROWS_PLAN_TABLE = [
    ("decode 64 256 1 8 1",            # few tokens, one piece, D = 64, f16 mask
     "attn_rows_decode_kernel<64> grid=8,1,1 block=1024 lds=5120 attr=0 S=0 chunk=256 ws=0 merge=0,0,0 m16=1 rows=1"),
    ("decode 128 960 3 8 0",           # the longest cache of one piece, D = 128, f32 mask
     "attn_rows_decode_kernel<128> grid=8,3,1 block=1024 lds=12032 attr=0 S=0 chunk=960 ws=0 merge=0,0,0 m16=0 rows=1"),
    ("decode 128 1024 1 32 1",         # the first cut cache
     "attn_rows_decode_kernel<128>;attn_combine_kernel grid=32,1,4 block=1024 lds=9216 attr=0 S=4 chunk=256 ws=66560 merge=32,1,256 m16=1 rows=1"),
    ("decode 64 1088 2 8 1",           # ragged pieces: 4 of 272
     "attn_rows_decode_kernel<64>;attn_combine_kernel grid=8,2,4 block=1024 lds=5184 attr=0 S=4 chunk=272 ws=16896 merge=8,2,256 m16=1 rows=1"),
    ("decode 128 16384 8 8 1",         # the longest cache: 16 pieces of 1024
     "attn_rows_decode_kernel<128>;attn_combine_kernel grid=8,8,16 block=1024 lds=12288 attr=0 S=16 chunk=1024 ws=532480 merge=8,8,256 m16=1 rows=1"),
    ("decode 128 4096 1 8 1 SPLIT=0",  # the switch: one workgroup walks the cache
     "attn_rows_decode_kernel<128> grid=8,1,1 block=1024 lds=24576 attr=0 S=0 chunk=4096 ws=0 merge=0,0,0 m16=1 rows=1"),
    ("decode 128 16384 1 8 1 SPLIT=0", # ... and past 64 KiB of scores the LDS limit is raised
     "attn_rows_decode_kernel<128> grid=8,1,1 block=1024 lds=73728 attr=1 S=0 chunk=16384 ws=0 merge=0,0,0 m16=1 rows=1"),
    ("prefill 64 64 20 8 1",           # prompt, one chunk, under 64 KiB
     "attn_rows_prefill_kernel<64> grid=1,8,1 block=256 lds=35840 attr=0 S=0 chunk=0 ws=0 merge=0,0,0 m16=1 rows=1"),
    ("prefill 128 128 70 8 0",
     "attn_rows_prefill_kernel<128> grid=2,8,1 block=256 lds=52224 attr=0 S=0 chunk=0 ws=0 merge=0,0,0 m16=0 rows=1"),
    ("prefill 128 256 9 8 1",          # one chunk, LDS limit raised
     "attn_rows_prefill_kernel<128> grid=1,8,1 block=256 lds=84992 attr=1 S=0 chunk=0 ws=0 merge=0,0,0 m16=1 rows=1"),
    ("prefill 128 512 512 32 1",       # a full chunk
     "attn_rows_prefill_kernel<128> grid=8,32,1 block=256 lds=150528 attr=1 S=0 chunk=0 ws=0 merge=0,0,0 m16=1 rows=1"),
    ("prefill 64 576 64 8 1",          # several chunks
     "attn_rows_prefill_kernel<64> grid=1,8,1 block=256 lds=150528 attr=1 S=0 chunk=0 ws=0 merge=0,0,0 m16=1 rows=1"),
    ("prefill 128 2304 130 8 1",
     "attn_rows_prefill_kernel<128> grid=3,8,1 block=256 lds=150528 attr=1 S=0 chunk=0 ws=0 merge=0,0,0 m16=1 rows=1"),
]


@pytest.fixture(scope="module")
def rows_plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each shape on its input"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("attnrowsplan")
    (d / "probe.cpp").write_text(ROWS_PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{ATTN_PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_rows_plan_keeps_every_decision(rows_plan_probe):
    got = rows_plan_probe([spec for spec, _ in ROWS_PLAN_TABLE])
    assert len(got) == len(ROWS_PLAN_TABLE)
    for (spec, want), line in zip(ROWS_PLAN_TABLE, got):
        assert line == want, spec


@pytest.fixture(scope="module")
def lib():
    from ggml_hexagon_amd import build, capi
    lib = ctypes.CDLL(str(build.build_qmm()))
    P = ctypes.POINTER(capi.QmmTensor)
    lib.qmm_attn_decode_supported.argtypes = [P, P, P, P, P]
    lib.qmm_attn_prefill_supported.argtypes = [P, P, P, P, P]
    return lib


def _ask(fn, ts):
    return fn(*[ctypes.byref(t) for t in ts])


F32, F16 = 0, 1
D, H, HK = 128, 8, 2


def _llama(d, n_tok, h, hk, n_kv, n_ctx=4096, **kw):
    """llama.cpp's operands: K / V strided views of an [n_ctx, hk * d] cache, q the permuted view of [d, h, n_tok], the mask padded to 64 rows"""
    from ggml_hexagon_amd import capi
    args = dict(q_nb=[4, h * d * 4, d * 4], k_nb=[2, hk * d * 2, d * 2], v_nb=[2, hk * d * 2, d * 2], mask_rows=(n_tok + 63) // 64 * 64)
    args.update(kw)
    return capi.flash_attn_operands(d, n_tok, h, hk, n_kv, q=1 << 20, k=2 << 20, v=3 << 20, mask=4 << 20, dst=5 << 20, **args)


def test_kv_rows_operands_are_taken(lib):
    from ggml_hexagon_amd import capi
    for mask_type in (F16, F32):
        for d in (64, 128):
            assert _ask(lib.qmm_attn_decode_supported, _llama(d, 1, H, HK, 256, mask_type=mask_type)) == 1
            assert _ask(lib.qmm_attn_decode_supported, _llama(d, 8, H, HK, 16384, n_ctx=16384, mask_type=mask_type)) == 1
            assert _ask(lib.qmm_attn_prefill_supported, _llama(d, 9, H, HK, 256, mask_type=mask_type)) == 1
            assert _ask(lib.qmm_attn_prefill_supported, _llama(d, 1, H, HK, 256, mask_type=mask_type)) == 1        # any N
            assert _ask(lib.qmm_attn_prefill_supported, _llama(d, 512, H, HK, 32768, n_ctx=32768, mask_type=mask_type)) == 1
            # contiguous [d, n_kv, hk] K / V and [d, n_tok, h] q, as test-backend-ops makes them; H_kv = H
            c = capi.flash_attn_operands(d, 3, 4, 4, 512, mask_type=mask_type, mask_rows=64)
            assert _ask(lib.qmm_attn_decode_supported, c) == 1 and _ask(lib.qmm_attn_prefill_supported, c) == 1
    # every multiple of 64 cache rows, nothing in between
    assert _ask(lib.qmm_attn_decode_supported, _llama(D, 2, H, HK, 64)) == 1 and _ask(lib.qmm_attn_prefill_supported, _llama(D, 70, H, HK, 576)) == 1
    assert _ask(lib.qmm_attn_decode_supported, _llama(D, 2, H, HK, 96)) == 0 and _ask(lib.qmm_attn_prefill_supported, _llama(D, 70, H, HK, 544)) == 0


def test_kv_rows_operands_outside_the_surface_are_refused(lib):
    both = (lib.qmm_attn_decode_supported, lib.qmm_attn_prefill_supported)
    for fn in both:
        assert _ask(fn, _llama(80, 2, H, HK, 256)) == 0                                         # D = 80
        assert _ask(fn, _llama(256, 2, H, HK, 256)) == 0                                        # D = 256
        ts = _llama(D, 2, H, HK, 256)
        ts[2].ne[0] = 64                                                                        # Dv != D
        ts[4].ne[0] = 64 * H
        assert _ask(fn, ts) == 0
        assert _ask(fn, _llama(D, 2, H, HK, 256, v_nb=[2, HK * D * 2 + 8, D * 2])) == 0         # V row stride off 16 bytes
        assert _ask(fn, _llama(D, 2, H, HK, 256, k_nb=[2, HK * D * 2, D * 2 + 4])) == 0         # K head stride off 16 bytes
        assert _ask(fn, _llama(D, 2, H, HK, 256, v_nb=[4, HK * D * 2, D * 2])) == 0             # V rows not dense
        assert _ask(fn, _llama(D, 2, H, 3, 256)) == 0                                           # H no multiple of H_kv
        ts = _llama(D, 2, H, HK, 256)
        ts[2].flags = 3                                                                         # a flag nobody defined
        assert _ask(fn, ts) == 0
        ts = _llama(D, 2, H, HK, 256)
        ts[2].type = 8                                                                          # a Q8_0 V cache
        assert _ask(fn, ts) == 0
        ts = _llama(D, 2, H, HK, 256)
        ts[3].type = 30                                                                         # a BF16 mask
        assert _ask(fn, ts) == 0
    assert _ask(lib.qmm_attn_decode_supported, _llama(D, 9, H, HK, 256)) == 0                   # 9 tokens on the few-token entry
    assert _ask(lib.qmm_attn_prefill_supported, _llama(D, 70, H, HK, 256, mask_rows=64)) == 0   # f16 mask rows fewer than N
    assert _ask(lib.qmm_attn_decode_supported, _llama(D, 8, H, HK, 256, mask_rows=4)) == 0
    assert _ask(lib.qmm_attn_prefill_supported, _llama(D, 9, H, HK, 256, q_nb=[4, H * D * 4 + 8, D * 4])) == 0    # q rows off 16 bytes (float4 loads)
    assert _ask(lib.qmm_attn_decode_supported, _llama(D, 2, H, HK, 16384 + 64, n_ctx=32768)) == 0                 # past the few-token limit ...
    assert _ask(lib.qmm_attn_prefill_supported, _llama(D, 2, H, HK, 16384 + 64, n_ctx=32768)) == 1               # ... the prompt entry takes it


def test_transposed_operands_answer_as_before(lib):
    """flags = 0: the transposed V cache, an f32 mask, the limits of the two existing families; the KV_ROWS rules do not leak into them"""
    from ggml_hexagon_amd.capi import QmmTensor as T

    def transposed(d, n_tok, n_kv, dv=None, mask_type=F32, n_ctx=4096):
        dv = dv or d
        return (T.make(F32, [d, n_tok, H], nb=[4, H * d * 4, d * 4, n_tok * H * d * 4]), T.make(F16, [d, n_kv, HK], nb=[2, HK * d * 2, d * 2, n_ctx * HK * d * 2]),
                T.make(F16, [n_kv, dv, HK], nb=[2, n_ctx * 2, n_ctx * dv * 2, n_ctx * dv * HK * 2]), T.make(mask_type, [n_kv, 128]), T.make(F32, [dv * H, n_tok]))
    dec, pre = lib.qmm_attn_decode_supported, lib.qmm_attn_prefill_supported
    assert _ask(dec, transposed(128, 1, 264)) == 1 and _ask(dec, transposed(256, 3, 640)) == 1 and _ask(dec, transposed(64, 2, 264, dv=192)) == 1
    assert _ask(dec, transposed(128, 9, 256)) == 0 and _ask(dec, transposed(128, 1, 260)) == 0 and _ask(dec, transposed(80, 1, 256)) == 0
    assert _ask(pre, transposed(128, 70, 96)) == 1 and _ask(pre, transposed(64, 33, 2080)) == 1
    assert _ask(pre, transposed(256, 70, 96)) == 0 and _ask(pre, transposed(128, 70, 72)) == 0 and _ask(pre, transposed(64, 33, 64, dv=128)) == 0
    assert _ask(dec, transposed(128, 1, 256, mask_type=F16)) == 0 and _ask(pre, transposed(128, 70, 256, mask_type=F16)) == 0      # the f16 mask comes with KV_ROWS only
    # the same descriptors read as KV_ROWS are another tensor (v [n_kv, dv, hk] would be rows of n_kv halves): refused, not reinterpreted
    ts = transposed(128, 1, 256)
    ts[2].flags = 1
    assert _ask(dec, ts) == 0 and _ask(pre, ts) == 0


def test_header_defines_the_flag_the_binding_uses():
    from ggml_hexagon_amd import capi
    import re
    m = re.search(r"#define\s+QMM_TENSOR_KV_ROWS\s+(\d+)", (ROOT / "include" / "ggml_mi355x_ops.h").read_text())
    assert m and int(m.group(1)) == capi.TENSOR_KV_ROWS == 1
