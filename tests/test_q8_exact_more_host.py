"""Host side of QMM_PREC_Q8_EXACT on Q2_K / Q3_K / IQ4_XS (no GPU): what the prefill plan decides for them, the integer helpers the
three Q8xBlock units call, enumerated over every (sc, q) pair, and the kernel's arithmetic restated in numpy (tests/q8x_refs.py) against
the CPU oracle on the very inputs of tests/test_gpu_q8_exact_more.py.  The last part is the check that the 2e-5 bar is reachable at all
with one f32 step per superblock: the CPU backend's Q3_K arm keeps eight f32 lanes and its scalar IQ4_XS arm makes one f32 term per
32-weight sub-block, so the f32 order differs although the integers do not."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import q8x_refs
from oracle.pyoracle import ACT_REF, TYPE_NAMES
from q8x_refs import BAR, IDS, MORE

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ggml-hexagon_amd" / "csrc"


def compile_probe(tmp_path_factory, name, text):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp(name)
    (d / "probe.cpp").write_text(text)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    return d / "probe"


# ---- the plan

PLAN_PROBE = r"""
#include "qmm_prefill_plan.h"
#include <cstdlib>
using namespace qmm;
static void line(const PrefillPlan & p) {
    printf("per_matrix=%d kernel=%d ta=%d tb=%d f16=%d grid=%u,%u,%u block=%u lds=%zu ksplit=%d wide=%d frag=%d tiles=%d,%d mtot=%d vec4=%d combine=%d reduce=%d "
           "label=%s act=%d perm=%d prep_reg=%d prep_q8x=%d x2=%d norm=%d prep_grid=%u prep_block=%u prep_lds=%zu tpw=%d Kp=%d key=%d unsupported=%s prep=%s "
           "o=%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu ws=%zu\n",
           (int) p.per_matrix, p.kernel, p.ta, p.tb, (int) p.f16, p.grid[0], p.grid[1], p.grid[2], p.block, p.lds, p.ksplit, p.wide, p.frag_major, p.tiles_x,
           p.n_tiles_y, p.mtot, (int) p.rows_vec4, (int) p.combine_ok, (int) p.reduce, p.label, p.act, p.perm, (int) p.prep_reg, (int) p.prep_q8x, (int) p.prep_x2,
           (int) p.prep_norm, p.prep_grid, p.prep_block, p.prep_lds, p.prep_tpw, p.Kp, p.key, p.unsupported ? p.unsupported : "-", p.prep_label,
           p.o_xh, p.o_scale, p.o_part, p.o_gather, p.o_dst_off, p.o_seg_start, p.o_seg_count, p.o_n_live, p.ws_total);
}
int main(int argc, char ** argv) {          // prec type M K N n_expert flags
    PrefillRules r = { 256, atoi(argv[1]), 1, 64, 128, 1, 0, 1 << 16, 1, 2, 1, 1, 1, 1 };      // qmm_ctx's defaults
    int64_t M = atoll(argv[3]);
    (void) argc;
    line(prefill_plan(r, atoi(argv[2]), &M, 1, atoll(argv[4]), atoll(argv[5]), atoll(argv[6]), (unsigned) atoi(argv[7])));
    printf("key=%d supported=%d\n", prefill_prep_key(r, atoi(argv[2]), M, atoll(argv[4]), atoll(argv[5])), (int) q8x_supports(atoi(argv[2]), atoll(argv[4])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_probe(tmp_path_factory, "q8x_more_plan", PLAN_PROBE)

    def run(prec, t, m, k, n, n_expert=1, flags=0):
        out = subprocess.run([str(exe)] + [str(v) for v in (prec, t, m, k, n, n_expert, flags)], check=True, capture_output=True, text=True).stdout.splitlines()
        fields = dict(f.split("=", 1) for f in out[0].split(" ") if "=" in f)
        return out[0], fields, out[1]
    return run


@pytest.mark.parametrize("t", MORE, ids=IDS)
@pytest.mark.parametrize("m,k,n", [(4096, 4096, 512), (200, 256, 9)])
def test_plan_of_the_exact_mode(plan, t, m, k, n):
    _, f, tail = plan(2, t, m, k, n)
    assert f["label"] == f"mfma_q8x_kernel<{t}>"
    assert f["prep"].startswith("prep_act_q8x_kernel") and f["prep_q8x"] == "1"
    assert f["grid"] == f"{(m + 127) // 128},{(n + 63) // 64},1" and f["block"] == "256" and f["ksplit"] == "1"
    assert tail == "key=1 supported=1"


@pytest.mark.parametrize("t", MORE, ids=IDS)
@pytest.mark.parametrize("k", [128, 384])
def test_k_off_the_superblock_is_the_default_plan(plan, t, k):
    assert plan(2, t, 200, k, 64)[0] == plan(1, t, 200, k, 64)[0]
    assert plan(2, t, 200, k, 64)[2] == plan(1, t, 200, k, 64)[2] and plan(2, t, 200, k, 64)[2].endswith("supported=0")
    assert "q8x" not in plan(2, t, 200, k, 64)[0].replace("prep_q8x=0", "")


def test_plan_of_mul_mat_id_is_the_default_modes(plan):
    assert plan(2, 10, 64, 512, 64, n_expert=4, flags=1)[0] == plan(1, 10, 64, 512, 64, n_expert=4, flags=1)[0]


# ---- the integer helpers, as the three units call them

SPLIT_PROBE = r"""
#include "qmm_q8x_split.h"
#include <cstdio>
using namespace qmm;
static const int kvalues[16] = { -127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113 };      // kvalues_iq4nl
struct Range { long bad; int hmin, hmax, vmin, vmax; };
// weight `q` at each of the four byte positions, the format's extremes and middle in the other three
template <typename F> static void each(const int * vals, int nv, int q, F f) {
    const int other[3] = { vals[0], vals[nv - 1], vals[nv / 2] };
    for (int pos = 0; pos < 4; ++pos) {
        int w[4];
        for (int j = 0, o = 0; j < 4; ++j) w[j] = j == pos ? q : other[o++];
        f(w);
    }
}
static void two_planes(Range & r, int sc, const int * w, uint32_t hi, uint32_t lo) {
    for (int j = 0; j < 4; ++j) {
        const int h = (int8_t) (hi >> (8 * j)), l = (int8_t) (lo >> (8 * j)), v = sc * w[j];
        if (128 * h + l != v || l < 0 || l > 127) ++r.bad;
        if (h < r.hmin) r.hmin = h;
        if (h > r.hmax) r.hmax = h;
        if (v < r.vmin) r.vmin = v;
        if (v > r.vmax) r.vmax = v;
    }
}
int main() {
    Range r = { 0, 1000, -1000, 1 << 20, -(1 << 20) };
    const int q3[8] = { -4, -3, -2, -1, 0, 1, 2, 3 };
    for (int sc = -32; sc <= 31; ++sc)                            // Q3_K: q8x_planes on (low bits | third bit << 2), bias 4
        for (int i = 0; i < 8; ++i)
            each(q3, 8, q3[i], [&](const int * w) {
                uint32_t packed = 0, hi, lo;
                for (int j = 0; j < 4; ++j) packed |= (uint32_t) (w[j] + 4) << (8 * j);
                q8x_planes(packed, 4, (short) sc, hi, lo);
                two_planes(r, sc, w, hi, lo);
            });
    printf("q3_K bad=%ld hi=%d..%d v=%d..%d\n", r.bad, r.hmin, r.hmax, r.vmin, r.vmax);
    r = { 0, 1000, -1000, 1 << 20, -(1 << 20) };
    for (int sc = -32; sc <= 31; ++sc)                            // IQ4_XS: q8x_planes_s8 on the table's bytes
        for (int i = 0; i < 16; ++i)
            each(kvalues, 16, kvalues[i], [&](const int * w) {
                uint32_t packed = 0, hi, lo;
                for (int j = 0; j < 4; ++j) packed |= (uint32_t) (uint8_t) (int8_t) w[j] << (8 * j);
                q8x_planes_s8(packed, (short) sc, hi, lo);
                two_planes(r, sc, w, hi, lo);
            });
    printf("iq4_xs bad=%ld hi=%d..%d v=%d..%d\n", r.bad, r.hmin, r.hmax, r.vmin, r.vmax);
    r = { 0, 0, 0, 1 << 20, -(1 << 20) };
    const int q2[4] = { 0, 1, 2, 3 };
    for (int sc = 0; sc <= 15; ++sc)                              // Q2_K: q8x_plane1, the one plane
        for (int i = 0; i < 4; ++i)
            each(q2, 4, q2[i], [&](const int * w) {
                uint32_t packed = 0;
                for (int j = 0; j < 4; ++j) packed |= (uint32_t) w[j] << (8 * j);
                const uint32_t p = q8x_plane1(packed, (uint32_t) sc);
                for (int j = 0; j < 4; ++j) {
                    const int v = (int8_t) (p >> (8 * j));
                    if (v != sc * w[j]) ++r.bad;
                    if (v < r.vmin) r.vmin = v;
                    if (v > r.vmax) r.vmax = v;
                }
            });
    printf("q2_K bad=%ld v=%d..%d\n", r.bad, r.vmin, r.vmax);
    return 0;
}
"""


def test_planes_of_every_scale_weight_pair(tmp_path_factory):
    """128 * hi + lo == sc * q with lo in [0, 127] and hi inside int8 for every pair Q3_K and IQ4_XS can hold; Q2_K's one plane == sc * q
    inside int8.  The ranges are those of the table at the top of qmm_q8x_split.h."""
    exe = compile_probe(tmp_path_factory, "q8x_more_split", SPLIT_PROBE)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out == ["q3_K bad=0 hi=-1..1 v=-124..128", "iq4_xs bad=0 hi=-31..31 v=-3937..4064", "q2_K bad=0 v=0..45"]


def test_the_edge_blocks_hold_what_their_names_say():
    for name, (t, blk, v) in q8x_refs.EDGES.items():
        planes = q8x_refs.unpack(t, blk[None, :], 256)[0]
        assert (planes == v).all(), (name, int(planes.min()), int(planes.max()))


# ---- the kernel's arithmetic against the CPU oracle, on the inputs of the GPU tests

def check(oracle, label, t, w, k, x):
    want = oracle.mul_mat(t, w, k, x, ACT_REF)
    assert np.isfinite(want).all()
    err = q8x_refs.rel_rms(q8x_refs.kernel_ref(oracle, t, w, k, x), want)
    print(TYPE_NAMES[t], label, err)
    assert err <= BAR, (label, err)


@pytest.mark.parametrize("t", MORE, ids=IDS)
def test_restated_kernel_meets_the_bar_on_the_parity_inputs(oracle, t):
    for n in q8x_refs.GRID_N:
        check(oracle, ("grid", n), t, *q8x_refs.grid_case(t, n))
    for shape in q8x_refs.RAGGED:
        check(oracle, shape, t, *q8x_refs.ragged_case(t, *shape))
    check(oracle, "strided", t, *q8x_refs.strided_case(t))
    check(oracle, "f16 top", t, *q8x_refs.f16_top_case(t))


@pytest.mark.parametrize("name", list(q8x_refs.EDGES))
def test_restated_kernel_meets_the_bar_on_the_range_edges(oracle, name):
    t, w, k, x = q8x_refs.edge_case(name)
    check(oracle, name, t, w, k, x)
