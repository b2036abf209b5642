"""CPU-side tests of MUL_MAT on BF16 weights (type 30): the numpy rounding of bf16_refs.py against hand-written cases, the launch plan
(csrc/qmm_bf16_plan.h) through a probe the host compiler builds from the header alone, and what the library answers about type 30
when it is loaded without a device."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bf16_refs as B

ROOT = Path(__file__).resolve().parents[1]
PLAN_HEADER = ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_bf16_plan.h"


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)


def test_rounding_is_ggml_compute_fp32_to_bf16():
    f = np.float32
    cases = [
        (f(1 + 2.0 ** -8), 0x3F80),             # a tie, even below: 1.0
        (f(1 + 3 * 2.0 ** -8), 0x3F82),         # a tie, odd below: up to 1 + 2^-6
        (f(-(1 + 2.0 ** -8)), 0xBF80),
        (f(1 + 2.0 ** -8 + 2.0 ** -23), 0x3F81),  # past the tie: up
        (f(-0.0), 0x8000),
        (_bits(0x7F7F0000)[0], 0x7F7F),         # the largest finite bf16 value stays
        (_bits(0x7F7FFFFF)[0], 0x7F80),         # the largest finite f32 value rounds up to infinity, as in ggml
        (_bits(0x00400000)[0], 0x0040),         # a subnormal (2^-127) is kept, not flushed
        (_bits(0x00018000)[0], 0x0002),         # ... and rounds to even like any other value
        (_bits(0x00000001)[0], 0x0000),
    ]
    for x, want in cases:
        got = int(B.f32_to_bf16(np.array([x], np.float32))[0])
        assert got == want, (float(x), hex(got), hex(want))
    assert B.bf16_to_f32(np.array([0x3F82], np.uint16))[0] == f(1 + 2.0 ** -6)
    assert B.bf16_to_f32(np.array([0x0040], np.uint16)).view(np.uint32)[0] == 0x00400000
    # the reference and its bound on a case small enough to check by hand: x = (1 + 2^-8, 2), w = (1, -0.5) -> 1 * 1 - 2 * 0.5 = 0
    want, absum = B.mul_mat_ref(B.f32_to_bf16(np.array([[1.0, -0.5] + [0.0] * 30], np.float32)), np.array([[1 + 2.0 ** -8, 2.0] + [0.0] * 30], np.float32))
    assert want[0, 0] == 0.0 and absum[0, 0] == 2.0 and B.bound(32, absum)[0, 0] == 2.0 ** -17


def test_synth_rows_are_the_same_rounding():
    from ggml_hexagon_amd import capi, synth
    assert capi.BF16 == 30 and synth.BF16 == 30 and synth.row_size(30, 4096) == 8192
    w = synth.synth_weights_bf16(5, 64, seed=3)
    assert w.dtype == np.uint16 and w.shape == (5, 64)
    x = (np.random.default_rng(3).standard_normal((5, 64)) * 0.02).astype(np.float32)
    assert np.array_equal(w, B.f32_to_bf16(x)) and np.array_equal(synth.f32_to_bf16(x), B.f32_to_bf16(x))


PLAN_PROBE = r"""
#include "qmm_bf16_plan.h"
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {       // mv cus rows K N | mm cus M N | w base_off row_bytes K M ldd | x base_off K N ldx | row K
        std::istringstream in(spec);
        std::string what;
        in >> what;
        if (what == "mv") {
            int cus; long long rows, K, N;
            in >> cus >> rows >> K >> N;
            const Bf16MvPlan p = bf16_matvec_plan(cus, rows, K, N);
            for (int k = 0; k < p.n; ++k) {
                const Bf16MvLaunch & l = p.launch[k];
                printf("%s%s n0=%d ntok=%d staged=%d lds=%zu attr=%d grid=%u block=%u", k ? " | " : "", l.label, l.n0, l.ntok, (int) l.staged, l.lds, (int) l.lds_attr, l.blocks, l.block);
            }
            printf("\n");
        } else if (what == "mm") {
            int cus; long long M, N;
            in >> cus >> M >> N;
            const Bf16MmPlan p = bf16_mfma_plan(cus, M, N);
            printf("%s tile=%d grid=%u,%u block=%u lds=%zu ksplit=%d ws=%zu\n", p.label, p.tile, p.grid[0], p.grid[1], p.block, p.lds, p.ksplit, p.ws_bytes);
        } else if (what == "w") {
            long long off, rb, K, M, ldd;
            in >> off >> rb >> K >> M >> ldd;
            const char * why = bf16_weight_refusal((const void *) (uintptr_t) (4096 + off), rb, K, M, ldd);
            printf("%s\n", why ? why : "ok");
        } else if (what == "x") {
            long long off, K, N, ldx;
            in >> off >> K >> N >> ldx;
            const char * why = bf16_src1_refusal((const float *) (uintptr_t) (4096 + off), K, N, ldx);
            printf("%s\n", why ? why : "ok");
        } else if (what == "row") {
            long long K;
            in >> K;
            printf("%zu\n", bf16_row_size(K));
        } else return 1;
    }
    return 0;
}
"""
# One line per branch, worked out by hand from the design, never printed by the header:
#   few tokens (256 CUs): a launch stages its tokens as bf16, 2 K bytes each, at most 128 KiB (131072 B) of them: the tokens of a call go
#   out floor(131072 / 2K) at a time; past 64 KiB (65536 B) the kernel's LDS limit is raised; a row that does not fit on its own (K > 65536)
#   is not staged, one token per launch.  Grid: rows per CU = ceil(rows / 256) -> 4 waves up to 4, 8 up to 8, else 16; one wave per row
#   in flight, at most one workgroup per CU.
#   prompt: 128 x 128 tiles when both M and N are past 64 and there are at least as many such tiles as CUs, else 64 x 64; LDS = 2 buffers x 2 operands x tile rows x 40 elements x 2 B;
#   no split-K, no workspace.
PLAN_TABLE = [
    ("mv 256 4096 4096 1", "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=8192 attr=0 grid=256 block=1024"),
    ("mv 256 4096 4096 8", "bf16_matvec_kernel<8,true> n0=0 ntok=8 staged=1 lds=65536 attr=0 grid=256 block=1024"),      # exactly 64 KiB: unasked
    ("mv 256 4096 4128 8", "bf16_matvec_kernel<8,true> n0=0 ntok=8 staged=1 lds=66048 attr=1 grid=256 block=1024"),      # one K-step more: limit raised
    ("mv 256 4096 8192 8", "bf16_matvec_kernel<8,true> n0=0 ntok=8 staged=1 lds=131072 attr=1 grid=256 block=1024"),     # exactly the budget
    ("mv 256 4096 8224 8",                                                                                                 # past it: 7 + 1
     "bf16_matvec_kernel<7,true> n0=0 ntok=7 staged=1 lds=115136 attr=1 grid=256 block=1024 | bf16_matvec_kernel<1,true> n0=7 ntok=1 staged=1 lds=16448 attr=0 grid=256 block=1024"),
    ("mv 256 64 14336 8",                                                                                                  # 8 x 14336 x 2 B = 224 KiB: two launches of four
     "bf16_matvec_kernel<4,true> n0=0 ntok=4 staged=1 lds=114688 attr=1 grid=16 block=256 | bf16_matvec_kernel<4,true> n0=4 ntok=4 staged=1 lds=114688 attr=1 grid=16 block=256"),
    ("mv 256 64 14336 5",
     "bf16_matvec_kernel<4,true> n0=0 ntok=4 staged=1 lds=114688 attr=1 grid=16 block=256 | bf16_matvec_kernel<1,true> n0=4 ntok=1 staged=1 lds=28672 attr=0 grid=16 block=256"),
    ("mv 256 64 14336 3", "bf16_matvec_kernel<3,true> n0=0 ntok=3 staged=1 lds=86016 attr=1 grid=16 block=256"),
    ("mv 256 64 65536 2",                                                                                                  # one token fills the budget
     "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=131072 attr=1 grid=16 block=256 | bf16_matvec_kernel<1,true> n0=1 ntok=1 staged=1 lds=131072 attr=1 grid=16 block=256"),
    ("mv 256 64 65568 2",                                                                                                  # ... and does not fit: unstaged
     "bf16_matvec_kernel<1,false> n0=0 ntok=1 staged=0 lds=0 attr=0 grid=16 block=256 | bf16_matvec_kernel<1,false> n0=1 ntok=1 staged=0 lds=0 attr=0 grid=16 block=256"),
    ("mv 256 1 32 1", "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=64 attr=0 grid=1 block=256"),
    ("mv 256 96 256 8", "bf16_matvec_kernel<8,true> n0=0 ntok=8 staged=1 lds=4096 attr=0 grid=24 block=256"),            # a group of 64 + 16 + 16 rows
    ("mv 256 1024 256 1", "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=512 attr=0 grid=256 block=256"),          # 4 rows per CU: 4 waves
    ("mv 256 1025 256 1", "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=512 attr=0 grid=129 block=512"),          # 5: 8 waves
    ("mv 256 2048 256 1", "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=512 attr=0 grid=256 block=512"),
    ("mv 256 2049 256 1", "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=512 attr=0 grid=129 block=1024"),         # 9: 16 waves
    ("mv 256 128256 4096 1", "bf16_matvec_kernel<1,true> n0=0 ntok=1 staged=1 lds=8192 attr=0 grid=256 block=1024"),     # never more workgroups than CUs
    ("mv 8 1057 4128 3", "bf16_matvec_kernel<3,true> n0=0 ntok=3 staged=1 lds=24768 attr=0 grid=8 block=1024"),
    ("mm 256 1 16", "bf16_mfma_kernel<64> tile=64 grid=1,1 block=256 lds=20480 ksplit=1 ws=0"),
    ("mm 256 64 9", "bf16_mfma_kernel<64> tile=64 grid=1,1 block=256 lds=20480 ksplit=1 ws=0"),
    ("mm 1 65 64", "bf16_mfma_kernel<64> tile=64 grid=2,1 block=256 lds=20480 ksplit=1 ws=0"),              # one CU: only the 64 | 65 rule is left
    ("mm 1 64 65", "bf16_mfma_kernel<64> tile=64 grid=1,2 block=256 lds=20480 ksplit=1 ws=0"),
    ("mm 1 65 65", "bf16_mfma_kernel<128> tile=128 grid=1,1 block=256 lds=40960 ksplit=1 ws=0"),
    ("mm 256 1057 130", "bf16_mfma_kernel<64> tile=64 grid=17,3 block=256 lds=20480 ksplit=1 ws=0"),          # 9 x 2 large tiles would leave 238 CUs idle
    ("mm 256 4096 512", "bf16_mfma_kernel<64> tile=64 grid=64,8 block=256 lds=20480 ksplit=1 ws=0"),          # 32 x 4 = 128 large tiles < 256 CUs
    ("mm 256 2048 1920", "bf16_mfma_kernel<64> tile=64 grid=32,30 block=256 lds=20480 ksplit=1 ws=0"),        # 16 x 15 = 240: still short
    ("mm 256 2048 2048", "bf16_mfma_kernel<128> tile=128 grid=16,16 block=256 lds=40960 ksplit=1 ws=0"),      # 256: every CU has one
    ("mm 256 2048 1921", "bf16_mfma_kernel<128> tile=128 grid=16,16 block=256 lds=40960 ksplit=1 ws=0"),      # a ragged 16th column of tiles counts
    ("mm 256 14336 512", "bf16_mfma_kernel<128> tile=128 grid=112,4 block=256 lds=40960 ksplit=1 ws=0"),
    ("mm 304 14336 512", "bf16_mfma_kernel<128> tile=128 grid=112,4 block=256 lds=40960 ksplit=1 ws=0"),
    # the surface: base and row stride on 16 bytes, K in whole steps of 32, a stride that holds the row, ldd >= M
    ("w 0 8192 4096 4096 4096", "ok"),
    ("w 0 528 256 1 1", "ok"),
    ("w 0 96 48 4 4", "BF16 weights: K must be a multiple of 32"),
    ("w 0 64 0 4 4", "BF16 weights: K must be a multiple of 32"),
    ("w 0 496 256 4 4", "BF16 weights: weight row stride < row size"),
    ("w 0 520 256 4 4", "BF16 weights: rows must start on 16-byte boundaries (base and row stride)"),
    ("w 8 512 256 4 4", "BF16 weights: rows must start on 16-byte boundaries (base and row stride)"),
    ("w 0 512 256 5 4", "BF16 weights: ldd < M"),
    ("x 0 256 3 256", "ok"),
    ("x 0 256 3 264", "ok"),
    ("x 0 256 3 252", "BF16 weights: src1 must be 16-byte aligned with ldx % 4 == 0 and ldx >= K"),
    ("x 0 256 3 258", "BF16 weights: src1 must be 16-byte aligned with ldx % 4 == 0 and ldx >= K"),
    ("x 4 256 3 256", "BF16 weights: src1 must be 16-byte aligned with ldx % 4 == 0 and ldx >= K"),
    ("row 4096", "8192"),
    ("row 32", "64"),
    ("row 100", "0"),
    ("row 1", "0"),
    ("row 0", "0"),
]


@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    """the plan header alone, compiled by the host compiler (no HIP, no ggml) into a program that prints the plan of each line of its input"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("bf16plan")
    (d / "probe.cpp").write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{PLAN_HEADER.parent}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return lambda specs: subprocess.run([str(d / "probe")], input="\n".join(specs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


def test_bf16_plan_keeps_every_decision(plan_probe):
    got = plan_probe([spec for spec, _ in PLAN_TABLE])
    assert len(got) == len(PLAN_TABLE)
    for (spec, want), line in zip(PLAN_TABLE, got):
        assert line == want, spec


def test_library_answers_for_type_30_without_a_device():
    from ggml_hexagon_amd import build
    lib = ctypes.CDLL(str(build.build_qmm()))
    lib.qmm_row_size.restype = ctypes.c_size_t
    lib.qmm_row_size.argtypes = [ctypes.c_int, ctypes.c_int64]
    lib.qmm_planar_type.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    lib.qmm_q8_exact_supported.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert lib.qmm_row_size(30, 4096) == 8192
    assert lib.qmm_row_size(30, 100) == 0
    assert lib.qmm_row_size(30, 32) == 64 and lib.qmm_row_size(30, 1) == 0
    assert lib.qmm_planar_type(30, 4096, 8192) == 0
    assert lib.qmm_q8_exact_supported(30, 4096) == 0
    assert lib.qmm_abi_version() == 2
