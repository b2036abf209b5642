"""Host side of the MUL_MAT_ID routing tests (no GPU): the launch plan of every shape case of tests/moe_cases.py, pinned field by field with
a probe on qmm_prefill_plan.h / qmm_matvec_plan.h under the host compiler (as test_host_logic.py and test_q8_exact_host.py do), and the
post-conditions of the routing generators.  test_gpu_moe_routing.py runs the same table and asserts the same labels through qmm.trace, so
this file is what keeps the table honest where there is no GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import moe_cases as mc
from oracle.pyoracle import Q2_K, Q3_K, TYPE_NAMES, WEIGHT_TYPES

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ggml-hexagon_amd" / "csrc"
IDS = [TYPE_NAMES[t] for t in WEIGHT_TYPES]
PREC_BF16, PREC_F16_Q8, PF_GATHER = 0, 1, 1

PROBE = r"""
#include "qmm_prefill_plan.h"
#include "qmm_matvec_plan.h"
using namespace qmm;
int main() {          // lines on stdin: "p prec regb_q23 type M K P n_expert"  or  "m form type K M P"
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'p') {
            int prec, q23, type;  long long M, K, P, ne;
            if (scanf("%d %d %d %lld %lld %lld %lld", &prec, &q23, &type, &M, &K, &P, &ne) != 7) return 1;
            PrefillRules r = { 256, prec, 1, 64, 128, 1, 0, 1 << 16, 1, 2, 1, 1, q23, 1 };      // qmm_ctx's defaults on 256 CUs
            int64_t m = M;
            const PrefillPlan p = prefill_plan(r, type, &m, 1, K, P, ne, PF_GATHER);
            printf("label=%s prep=%s frag=%d grid=%u,%u,%u ksplit=%d Kp=%d prep_grid=%u\n", p.label, p.prep_label, p.frag_major, p.grid[0], p.grid[1], p.grid[2],
                   p.ksplit, p.Kp, p.prep_grid);
        } else {
            int form, type, K, M, P;
            if (scanf("%d %d %d %d %d", &form, &type, &K, &M, &P) != 5) return 1;
            const MoeMatvecPlan p = moe_matvec_plan(256, form, type, K, M, P);
            char text[48];
            p.text(text, sizeof(text));
            printf("label=%s grid=%u,%u,%u block=%u runs_as_matvec=%d\n", text, p.grid[0], p.grid[1], p.grid[2], p.block, (int) moe_runs_as_matvec(1, P));
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("moe_plan")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "probe")], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [dict(f.split("=", 1) for f in l.split(" ")) for l in out]
    return run


def plan_line(prec, q23, t, case, k):
    return f"p {prec} {q23} {t} {case.M} {k} {mc.pairs(case)} {case.n_expert}"


def check(f, case, t, k, **prep):
    assert f["label"] == mc.label_of(case, t), (case.name, TYPE_NAMES[t], k, f)
    assert f["prep"] == mc.prep_label_of(case, t, k, **prep), (case.name, TYPE_NAMES[t], k, f)
    assert f["frag"] == ("1" if mc.kernel_of(case, t)[0] == "skinny" else "0")
    assert f["grid"] == ",".join(str(g) for g in mc.grid_of(case, t)), (case.name, TYPE_NAMES[t], k, f)
    assert f["ksplit"] == "1" and f["Kp"] == str((k + 127) // 128 * 128) and f["prep_grid"] == str(mc.pairs(case))


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_default_plan_of_every_case(probe, t):
    """label, prep label, operand layout, grid and ksplit == 1 of every (case, K) in the default precision"""
    todo = [(case, k) for case in mc.DEFAULT_CASES for k in mc.k_values(t)]
    for (case, k), f in zip(todo, probe([plan_line(PREC_F16_Q8, 1, t, case, k) for case, k in todo])):
        check(f, case, t, k)


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_bf16_plan_is_the_lds_tile_kernel(probe, t):
    todo = [(case, k) for case in mc.LDS_CASES for k in mc.k_values(t)]
    for (case, k), f in zip(todo, probe([plan_line(PREC_BF16, 1, t, case, k) for case, k in todo])):
        check(f, case, t, k, f16=False)


@pytest.mark.parametrize("t", (Q2_K, Q3_K), ids=["q2_K", "q3_K"])
def test_regb_q23_off_plan_is_the_lds_tile_kernel_in_f16(probe, t):
    todo = [(case, k) for case in mc.LDS_CASES for k in mc.k_values(t)]
    for (case, k), f in zip(todo, probe([plan_line(PREC_F16_Q8, 0, t, case, k) for case, k in todo])):
        check(f, case, t, k, regb_q23=False)


def test_pins_cover_every_gathered_variant():
    """every variant the plan can pick in gather mode is the label of some case, for a 64-wide and for a 128-wide type each (the
    128-token tile of four waves does not exist for the 128-wide units)"""
    def kinds(types, cases):
        return {mc.kernel_of(c, t) for c in cases for t in types}
    narrow = tuple(t for t in WEIGHT_TYPES if t not in mc.WIDE_UNITS)
    regb = {("skinny", 8, 1), ("skinny", 8, 2), ("regb", 4, 32), ("regb", 4, 64), ("regb", 8, 128)}
    assert kinds(narrow, mc.DEFAULT_CASES) == regb | {("regb", 4, 128)}
    assert kinds(mc.WIDE_UNITS, mc.DEFAULT_CASES) == regb
    for types in (narrow, mc.WIDE_UNITS):
        assert kinds(types, mc.LDS_CASES) == {("lds", 64, 128), ("lds", 128, 128)}
    assert mc.pairs(mc.BAD_ID_CASE) == 258 and mc.BAD_ID_CASE.n_expert >= 3
    assert {mc.pairs(c) for c in mc.DEFAULT_CASES if c.kernel == ("skinny", 8, 2)} == {60, 100}


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_few_pair_plan(probe, t):
    """K = 4352 is more than one wave of units for every type; grid[1] of the three forms, and where the row loop runs more than once"""
    forms = (0, 1, 2)                          # MOE_MV_SINGLE, MOE_MV_PAIR, MOE_MV_SWIGLU
    todo = [(k, fc, form) for k, fc in mc.few_k_cases(t) for form in forms]
    out = probe([f"m {form} {t} {k} {fc.M} {fc.n_tokens * fc.n_used}" for k, fc, form in todo])
    loops = {}
    # every type walks a second, full slice and a third, partial one: 136 = 64 + 64 + 8 units of 32, 132 = 64 + 64 + 4 units of 64
    assert max(k for k, _, _ in todo) // mc.mv_unit_width(t) in (136, 132)
    for (k, fc, form), f in zip(todo, out):
        P, nm = fc.n_tokens * fc.n_used, 2 if form == 1 else 1
        by = fc.grid_y[form]
        assert f["grid"] == f"{P},{by},{nm}" and f["block"] == "512" and f["runs_as_matvec"] == "1"
        assert f["label"] == ("matvec_id_swiglu_kernel<%d>" if form == 2 else "matvec_id_kernel<%d>") % t
        assert k // mc.mv_unit_width(t) in (68, 136, 132)                     # more than the 64 lanes of a wave: the second slice runs
        loops[(fc.M, P, form)] = -(-fc.M // (by * 8))
    # M = 41: six row chunks of 8 waves cover the rows in one pass; M = 300 at 16 pairs: grid[1] is capped, the row loop iterates
    assert all(n == 1 for (m, _, _), n in loops.items() if m == 41)
    assert loops[(300, 16, 0)] == 2 and loops[(300, 16, 1)] == 3 and loops[(300, 16, 2)] == 2


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_generators_keep_their_post_conditions(t):
    """every (case, pattern) of the GPU tests: the generators assert their own distribution; here also the segment lengths at the tile edge"""
    for case in mc.DEFAULT_CASES + mc.LDS_CASES:
        bn, P = mc.bn_of(case, t), mc.pairs(case)
        names = [n for n, _ in mc.patterns(case, t)]
        assert len(set(names)) == len(names)
        for name, gen in mc.patterns(case, t):
            ids = mc.make_ids(case, t, name, gen)
            assert np.array_equal(ids, mc.make_ids(case, t, name, gen))           # the same routing wherever it is asked for
            cnt = np.bincount(ids.ravel(), minlength=case.n_expert)
            if name.startswith("edge"):
                assert cnt[case.n_expert // 2] == int(name[5:-1])
            if name == "sparse":
                assert np.count_nonzero(cnt == 0) * 2 >= case.n_expert and case.n_expert == 64 and case.n_used == 6
        if case.n_expert >= 3:
            want = [c for c in (bn - 1, bn, bn + 1, 2 * bn + 1) if c <= P]
            assert list(mc.edge_counts(case, t)) == (want or [P - 3])
            assert want or P < bn - 1                                              # (a case of fewer pairs than its tile)
    for fc in mc.FEW_CASES:
        ids = mc.few_ids(fc)
        assert ids.shape == (fc.n_tokens, fc.n_used) and fc.n_tokens * fc.n_used <= 16
