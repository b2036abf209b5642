"""Host side of QMM_PREC_Q8_EXACT (no GPU): what the prefill plan decides in that mode, the switch parse, and the integer helper that
cuts sc * q into two int8 planes.  Each probe is the header alone under the host compiler, as in test_host_logic.py."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

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
    exe = compile_probe(tmp_path_factory, "q8x_plan", PLAN_PROBE)

    def run(prec, t, m, k, n, n_expert=1, flags=0):
        out = subprocess.run([str(exe)] + [str(v) for v in (prec, t, m, k, n, n_expert, flags)], check=True, capture_output=True, text=True).stdout.splitlines()
        fields = dict(f.split("=", 1) for f in out[0].split(" ") if "=" in f)
        return out[0], fields, out[1]
    return run


@pytest.mark.parametrize("t", [12, 13, 14])
@pytest.mark.parametrize("m,k,n", [(4096, 4096, 512), (200, 256, 9)])
def test_plan_of_the_exact_mode(plan, t, m, k, n):
    _, f, tail = plan(2, t, m, k, n)
    assert f["label"].startswith("mfma_q8x_kernel<") and f["label"] == f"mfma_q8x_kernel<{t}>"
    assert f["prep"].startswith("prep_act_q8x_kernel") and f["prep_q8x"] == "1"
    assert f["grid"] == f"{(m + 127) // 128},{(n + 63) // 64},1" and f["block"] == "256" and f["ksplit"] == "1"
    # the workspace holds the int8 operand [N, K] and its scales [N, K / 256] f32, one behind the other
    o_xh, o_scale, o_part = (int(v) for v in f["o"].split(",")[:3])
    assert o_scale - o_xh >= n * k and o_part - o_scale >= n * (k // 256) * 4 and int(f["ws"]) >= o_part > 0
    assert tail == "key=1 supported=1"


@pytest.mark.parametrize("t,m,k,n", [(t, m, k, n) for t in (2, 8, 114) for (m, k, n) in ((4096, 4096, 512), (200, 256, 9), (4096, 2048, 64))
                                     if t != 114 or k % 2048 == 0])           # (planar Q6_K rows exist for K % 2048 == 0)
def test_plan_of_other_types_is_the_default_modes(plan, t, m, k, n):
    """Q4_0, Q8_0 and planar Q6_K rows: field for field the QMM_PREC_F16_Q8 plan, and the same prep key"""
    assert plan(2, t, m, k, n)[0] == plan(1, t, m, k, n)[0]
    assert plan(2, t, m, k, n)[2] == plan(1, t, m, k, n)[2] and plan(2, t, m, k, n)[2].endswith("supported=0")
    assert "q8x" not in plan(2, t, m, k, n)[0].replace("prep_q8x=0", "")


def test_plan_of_mul_mat_id_is_the_default_modes(plan):
    assert plan(2, 12, 64, 512, 64, n_expert=4, flags=1)[0] == plan(1, 12, 64, 512, 64, n_expert=4, flags=1)[0]


def test_default_and_bf16_plans_do_not_know_the_mode(plan):
    for prec in (0, 1):
        line, f, _ = plan(prec, 12, 4096, 4096, 512)
        assert "q8x" not in line.replace("prep_q8x=0", "") and f["prep_q8x"] == "0"


# ---- the switch

SWITCH_PROBE = r"""
#include "qmm_switches.h"
#include <cstdio>
int main() {
    using namespace qmm_sw;
    const values v = read();
    printf("%d %d\n", (int) prec_is_q8(v.str(SW_PREC)), (int) prec_is_bf16(v.str(SW_PREC)));
    return 0;
}
"""


def test_prec_is_q8(tmp_path_factory):
    exe = compile_probe(tmp_path_factory, "q8x_switch", SWITCH_PROBE)
    base = {k: v for k, v in os.environ.items() if not k.startswith("GGML_MI355X_")}

    def run(value):
        env = dict(base) if value is None else dict(base, GGML_MI355X_PREC=value)
        return subprocess.run([str(exe)], env=env, check=True, capture_output=True, text=True).stdout.split()
    assert run("q8") == ["1", "0"] and run("2") == ["1", "0"]
    assert run("bf16") == ["0", "1"] and run("0") == ["0", "1"]
    for v in ("f16q8", "1", "Q8", "", None):
        assert run(v) == ["0", "0"], v


# ---- the integer helper

SPLIT_PROBE = r"""
#include "qmm_q8x_split.h"
#include <cstdio>
using namespace qmm;
// every (sc, q) pair of a format, four weights at a time through q8x_planes as the kernel calls it
static long check(int sc_lo, int sc_hi, int q_lo, int q_hi, int bias, int & hmin, int & hmax) {
    long bad = 0;
    for (int sc = sc_lo; sc <= sc_hi; ++sc)
        for (int q = q_lo; q <= q_hi; ++q) {
            const int other[3] = { q_lo, q_hi, (q_lo + q_hi) / 2 };
            for (int pos = 0; pos < 4; ++pos) {
                int w[4];
                for (int j = 0, o = 0; j < 4; ++j) w[j] = j == pos ? q : other[o++];
                uint32_t packed = 0, hi, lo;
                for (int j = 0; j < 4; ++j) packed |= (uint32_t) (w[j] + bias) << (8 * j);
                q8x_planes(packed, (short) bias, (short) sc, hi, lo);
                for (int j = 0; j < 4; ++j) {
                    const int h = (int8_t) (hi >> (8 * j)), l = (int8_t) (lo >> (8 * j));
                    if (128 * h + l != sc * w[j] || l < 0 || l > 127) ++bad;
                    if (h < hmin) hmin = h;
                    if (h > hmax) hmax = h;
                }
            }
        }
    return bad;
}
int main() {
    const struct { const char * name; int sc_lo, sc_hi, q_lo, q_hi, bias; } f[3] = {
        { "q4_K", 0, 63, 0, 15, 0 }, { "q5_K", 0, 63, 0, 31, 0 }, { "q6_K", -128, 127, -32, 31, 32 } };
    for (int i = 0; i < 3; ++i) {
        int hmin = 1000, hmax = -1000;
        const long bad = check(f[i].sc_lo, f[i].sc_hi, f[i].q_lo, f[i].q_hi, f[i].bias, hmin, hmax);
        printf("%s bad=%ld hi=%d..%d\n", f[i].name, bad, hmin, hmax);
    }
    return 0;
}
"""


def test_hi_lo_split_of_every_scale_weight_pair(tmp_path_factory):
    """128 * hi + lo == sc * q with lo in [0, 127] and hi inside int8, for every pair the three formats can hold"""
    exe = compile_probe(tmp_path_factory, "q8x_split", SPLIT_PROBE)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out == ["q4_K bad=0 hi=0..7", "q5_K bad=0 hi=0..15", "q6_K bad=0 hi=-32..32"]


# ---- the public surface

def test_header_and_binding_name_the_mode():
    header = (ROOT / "include" / "ggml_mi355x_qmm.h").read_text()
    assert "QMM_PREC_Q8_EXACT = 2" in header and "qmm_q8_exact_supported(int type, int64_t K)" in header
    from ggml_hexagon_amd import capi
    assert capi.PREC_Q8_EXACT == 2 and "qmm_q8_exact_supported" in capi.EXPORTS
