"""Host side of the plain MUL_MAT prefill branch tests (no GPU): the launch plan of every case of tests/mulmat_cases.py, pinned field by field
with a probe on qmm_prefill_plan.h under the host compiler (as test_moe_routing_host.py does for the gathered half), the split-K range
lengths the table writes out against the kernels' formula, and the coverage the table promises.  test_gpu_mulmat_branches.py runs the same
table and asserts the same labels through qmm.trace, so this file is what keeps the table honest where there is no GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

import mulmat_cases as mm
from oracle.pyoracle import Q4_K, TYPE_NAMES, WEIGHT_TYPES

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ggml-hexagon_amd" / "csrc"
IDS = [TYPE_NAMES[t] for t in WEIGHT_TYPES]

PROBE = r"""
#include "qmm_prefill_plan.h"
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
using namespace qmm;
int main() {
    std::string spec;
    while (std::getline(std::cin, spec)) {          // type M1,M2,.. K N [NAME=VAL ...]
        std::istringstream in(spec);
        PrefillRules r = {};                         // qmm_ctx's defaults on 256 CUs, field by field: a new field cannot shift them
        r.cus = 256;  r.prec = QMM_PREC_F16_Q8;  r.skinny = 1;  r.skinny_max_n = 64;  r.skinny_max_n_few = 128;  r.splitk = 1;  r.splitk_combine = 0;
        r.kcnt_n = 1 << 16;  r.wide = 1;  r.r64 = 2;  r.r64s = 1;  r.prep_reg = 1;  r.regb_q23 = 1;  r.mm_group = 1;
        int type; int64_t K, N; std::string ms, kv;
        in >> type >> ms >> K >> N;
        qmm_weight ws[4] = {};
        int nw = 0;
        { std::istringstream m(ms); std::string x; while (nw < 4 && std::getline(m, x, ',')) { ws[nw].type = type; ws[nw].M = atoll(x.c_str()); ++nw; } }
        while (in >> kv) {
            const std::string name = kv.substr(0, kv.find('=')); const int v = atoi(kv.c_str() + kv.find('=') + 1);
            if (name == "R64") r.r64 = v; else if (name == "R64S") r.r64s = v; else if (name == "SPLITK_COMBINE") r.splitk_combine = v;
            else if (name == "BF16") r.prec = v ? QMM_PREC_BF16 : QMM_PREC_F16_Q8; else return 1;
        }
        PrefillGroupPlan g;
        prefill_group_plan(g, r, ws, nw, K, N, 0);
        if (g.error) return 2;
        for (int k = 0; k < g.n; ++k) {
            const PrefillEntry & e = g.e[k];
            const PrefillPlan & p = e.plan;
            if (p.per_matrix) return 3;
            printf("%sfirst=%d n=%d prep=%d label=%s prep_label=%s ksplit=%d reduce=%d combine=%d wide=%d grid=%u,%u,%u Kp=%d vec4=%d frag=%d o_part=%zu", k ? ";" : "", e.first, e.n,
                   (int) e.prep, p.label, p.prep_label, p.ksplit, (int) p.reduce, (int) p.combine_ok, p.wide, p.grid[0], p.grid[1], p.grid[2], p.Kp, (int) p.rows_vec4,
                   p.frag_major, p.o_part);
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("mulmat_plan")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "probe")], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[dict(f.split("=", 1) for f in e.split(" ")) for e in l.split(";")] for l in out]
    return run


def plan_line(t, case, Ms=None):
    _, switches, bf16 = mm.CONTEXTS[case.ctx]
    return f"{t} {','.join(str(m) for m in Ms or case.Ms)} {case.K} {case.N} {switches}" + (" BF16=1" if bf16 else "")


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_plan_of_every_case(probe, t):
    """per launch of every case: which matrices, whether it prepares, label (with +combine), prep label, ksplit, reduce / combine, wide, grid"""
    todo = mm.cases(t)
    assert len({c.name for c in todo}) == len(todo)
    for case, entries in zip(todo, probe([plan_line(t, c) for c in todo])):
        where = (TYPE_NAMES[t], case.name, entries)
        assert len(entries) == len(case.launches), where
        for l, e in zip(case.launches, entries):
            assert (int(e["first"]), int(e["n"]), e["prep"]) == (l.first, l.n, "1" if l.prep else "0"), where
            assert e["label"] + ("+combine" if e["combine"] == "1" else "") == mm.label_of(l, t), where
            assert e["prep_label"] == mm.prep_label_of(case, t), where
            assert int(e["ksplit"]) == l.ksplit and e["wide"] == ("1" if l.wide else "0"), where
            # the plan's `reduce` says split-K slabs exist; the reduce kernel runs unless the launch combines them itself
            assert (e["reduce"] == "1") == (l.ksplit > 1) and (e["combine"] == "1") == l.combine and l.reduce == (l.ksplit > 1 and not l.combine), where
            assert e["grid"] == ",".join(str(g) for g in l.grid), where
            assert e["Kp"] == str(mm.kpad(case.K)) and e["frag"] == ("1" if l.kernel[0] == "skinny" else "0"), where
            assert (e["vec4"] == "1") == all(m % 4 == 0 for m in case.Ms[l.first:l.first + l.n]), where
        assert sum(l.n for l in case.launches) == len(case.Ms) and mm.out_elements(case) <= mm.MAX_OUT, where
        # a combined launch needs destinations it can store whole float4 to: the GPU test lays them out ldd = M + 12 apart
        assert not any(l.combine for l in case.launches) or all(m % 4 == 0 for m in case.Ms), where


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_dirtying_launch_covers_the_slabs_of_its_case(probe, t):
    """every case with an empty or a past-the-end range has a dirtying launch (mulmat_cases.dirty_rows): split-K too, its slabs at the case's
    offset in the workspace, its first range with work, and its slab 0 (N x rows floats) no smaller than all slabs of the case together"""
    todo = [c for c in mm.cases(t) if mm.dirty_rows(c)]
    assert {mm.range_class(c.ranges) for c in todo} == {"empty", "past-end"}
    assert all(mm.dirty_rows(c) for c in mm.cases(t) if c.ranges and min(c.ranges) <= 0) and len(todo) >= 4
    small, big = probe([plan_line(t, c) for c in todo]), probe([plan_line(t, c, (mm.dirty_rows(c),)) for c in todo])
    for case, (s,), b in zip(todo, small, big):
        where = (TYPE_NAMES[t], case.name, b)
        assert len(b) == 1 and int(b[0]["ksplit"]) > 1 and b[0]["reduce"] == "1" and b[0]["o_part"] == s["o_part"], where
        assert mm.range_lengths(t, case.K, int(b[0]["ksplit"]))[0] > 0, where
        assert mm.dirty_rows(case) >= int(s["ksplit"]) * sum(case.Ms) and mm.DIRTY_FACTOR * mm.out_elements(case) <= mm.MAX_OUT, where


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_range_lengths_as_written(t):
    """the range lengths the table writes out are what the kernels' formula gives for the pinned ksplit; cases without split-K name none"""
    for case in mm.cases(t):
        split = [l for l in case.launches if l.ksplit > 1]
        assert len(split) <= 1
        if split:
            assert case.ranges == mm.range_lengths(t, case.K, split[0].ksplit), (TYPE_NAMES[t], case.name)
            assert len(case.ranges) == split[0].grid[2] == split[0].ksplit
        else:
            assert case.ranges is None, (TYPE_NAMES[t], case.name)


def test_range_formula_on_known_shapes():
    """the restated formulas against lengths worked out by hand from the kernel source: Q4_0 K = 1056 is 18 K-steps of 64 on the padded row,
    two ranges of ((9 + 1) & ~1) = 10: 10 and 8; Q6_K K = 2304 is 18 K-steps of 128, four ranges of 6: the last is empty; Q4_K M = K = 5120 at
    200 tokens (a real shape) is 20 blocks cut 6 ways by 4: the last range is empty"""
    from oracle.pyoracle import Q4_0, Q6_K
    assert mm.range_lengths(Q4_0, 1056, 2) == (10, 8)
    assert mm.range_lengths(Q4_0, 4160, 8) == (10, 10, 10, 10, 10, 10, 6, -4)
    assert mm.range_lengths(Q6_K, 2304, 4) == (6, 6, 6, 0)
    assert mm.range_lengths(Q6_K, 4352, 8) == (6, 6, 6, 6, 6, 4, -2, -8)
    assert mm.range_lengths(Q4_K, 4352, 8) == (3, 3, 3, 3, 3, 2, -1, -4)
    assert mm.range_lengths(Q4_K, 5120, 6) == (4, 4, 4, 4, 4, 0)
    assert [mm.range_class(r) for r in ((8, 8), (10, 8), (6, 6, 6, 0), (6, 4, -2, -8), None)] == ["even", "ragged", "empty", "past-end", None]


def test_every_range_class_on_every_kernel_family():
    """for the generic kernel at BK = 64 and at BK = 128, for the Q4_K kernel and for mfma_r64_q4k_kernel<4>: an even split, a ragged last
    range, an empty last range and a range that begins past the end of K, each on the reduce kernel; the scalar and the float4 reduce both see
    an empty and a past-the-end range; the in-launch combine sees an empty range, alone and in a group"""
    every = {"even", "ragged", "empty", "past-end"}
    seen = {}
    for t in WEIGHT_TYPES:
        for case in mm.cases(t):
            for l in case.launches:
                if l.ksplit > 1:
                    key = (l.kernel[0], mm.bk(t) if l.kernel[0] == "regb" and t != Q4_K else "q4k", "combine" if l.combine else
                           "reduce-vec4" if all(m % 4 == 0 for m in case.Ms) else "reduce-scalar")
                    seen.setdefault(key, set()).add(mm.range_class(case.ranges))
    for unit in (64, 128, "q4k"):
        assert seen[("regb", unit, "reduce-vec4")] == every, (unit, seen)
        assert {"empty", "past-end"} <= seen[("regb", unit, "reduce-scalar")], (unit, seen)
    assert seen[("r64", "q4k", "reduce-vec4")] == every and "empty" in seen[("r64", "q4k", "reduce-scalar")], seen
    for unit in (128, "q4k"):
        assert "empty" in seen[("regb", unit, "combine")], seen
    assert "ragged" in seen[("regb", 64, "combine")], seen


def test_table_covers_every_branch():
    """every kernel variant the plan can pick for a plain MUL_MAT, the register prep and the LDS prep, one launch over a group and one per
    matrix, for the 64-wide and for the 128-wide units"""
    def kinds(types):
        return {l.kernel for t in types for c in mm.cases(t) for l in c.launches}
    narrow = tuple(t for t in WEIGHT_TYPES if t not in mm.WIDE_UNITS)
    common = {("skinny", 8, 1), ("skinny", 8, 2), ("regb", 4, 32), ("regb", 4, 64), ("regb", 8, 128), ("lds", 64, 0), ("lds", 128, 0)}
    assert kinds(mm.WIDE_UNITS) == common
    assert kinds(t for t in narrow if t != Q4_K) == common | {("regb", 4, 128)}
    assert kinds((Q4_K,)) == common | {("regb", 4, 128), ("r64", 4, 0), ("r64", 8, 0), ("r64s", 2, 0), ("wide", 8, 0)}
    for t in WEIGHT_TYPES:
        cs = mm.cases(t)
        preps = {mm.prep_label_of(c, t) for c in cs}
        assert any(p.startswith("prep_act_kernel") for p in preps)
        assert any(p.startswith("prep_act_q8k_kernel") for p in preps) == (mm.family(t) != "b32" and TYPE_NAMES[t] != "iq4_xs")
        assert any(len(c.launches) == 1 and c.launches[0].n == 3 for c in cs) and any(len(c.launches) == 2 and not c.launches[1].prep for c in cs)
        assert {c.ctx for c in cs} >= {"default", "combine", "bf16"} and all(c.ctx in mm.CONTEXTS for c in cs)
        assert all(c.repeat == (4 if c.ctx == "combine" else 1) for c in cs)
