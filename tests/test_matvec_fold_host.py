"""The case table of the mat-vec folds (tests/matvec_fold_cases.py) without a GPU: the launch plan of every case, pinned through the host probe
on csrc/qmm_matvec_plan.h (the probe of test_host_logic.py); what the table covers; the LDS invariant of the fit estimates; and the
rounding-stable activation rows of tests/helpers.py against the C oracle's quantizers."""
import numpy as np
import pytest

import helpers as H
import matvec_fold_cases as F
from test_host_logic import mv_plan_probe  # noqa: F401  (the fixture: the plan header compiled by the host compiler)

ALL = F.all_cases()


# ---- plan pins

# (spec, what the plan header has to print), worked out by hand from the header's rules (mv_act_bytes, matvec_launch, matvec_group_plan):
#   Q4_K, 6 x 4096 with the norm: 24576 values + 6 x 16 x 4 scales + 6 x 128 x 2 sums = 26496, + 98304 of f32 rows; 72 rows: 4 waves, 18 blocks
#   Q5_1, 5 x 5120 with the norm: 25600 + 3200 (d) + 3200 (s) = 32000, + 102400
#   Q3_K (sums per 16), 1 x 4096 with the norm: 4096 + 64 + 512 = 4672, + 16384; 2304 rows: 9 per CU, 16 waves, 144 blocks; 1280: 8 waves, 160
#   IQ4_XS, SwiGLU with the norm, 6 x 4096: 24576 + 384 + 3072 = 28032, + 98304; the pair counts as 24 rows
#   Q5_0, 7 x 28672 with a residual: 4 tokens at once (7 -> 4), 114688 + 14336 = 129024, then 3: 86016 + 10752 = 96768
#   Q4_K + Q8_0 + Q8_0P with residuals, 4 x 4096: 16384 + 256 + 2048 = 18688 (Q8_K, sums per 16), + 16384 + 2048 (Q8_0) = 37120; at 5 tokens
#   one run per type: Q4_K 20480 + 320 + 1280 = 22080, Q8_0 20480 + 2560 = 23040
#   the mixed K-quant group, 2 x 1024 with the norm, one-pass staging off: 2048 + 32 + 256 = 2336, + 8192; the argument carries bit 8
HAND_PINS = [
    ("group 256 12,12,12 40,24,8 4096 6 n",
     "matvec_kernel<12,6,true> m=0:40,1:64,2:72 n0=0 grid=18 block=256 lds=124800 arg=0"),
    ("group 256 7,7,7 40,24,8 5120 5 n",
     "matvec_kernel<7,5,true> m=0:40,1:64,2:72 n0=0 grid=18 block=256 lds=134400 arg=0"),
    ("group 256 11 2304 4096 1 n",
     "matvec_kernel<11,1,true> m=0:2304 n0=0 grid=144 block=1024 lds=21056 arg=0"),
    ("group 256 11 1280 4096 1 n",
     "matvec_kernel<11,1,true> m=0:1280 n0=0 grid=160 block=512 lds=21056 arg=0"),
    ("group 256 11 40 4096 1 n",
     "matvec_kernel<11,1,true> m=0:40 n0=0 grid=10 block=256 lds=21056 arg=0"),
    ("group 256 23,23 24,24 4096 6 ns2",
     "matvec_kernel<23,6,true> m=0:24,1:48 n0=0 grid=6 block=256 lds=126336 arg=0"),
    ("group 256 6 8 28672 7 r0",
     "matvec_kernel<6,4,true> m=0:8 n0=0 grid=2 block=256 lds=129024 arg=0; matvec_kernel<6,3,true> m=0:8 n0=4 grid=2 block=256 lds=96768 arg=0"),
    ("group 256 12,8,108 40,24,8 4096 4 r0r1r2",
     "matvec_kmix_kernel<4,true,q8_0> m=0:40,1:64,2:72 n0=0 grid=18 block=256 lds=37120 arg=0"),
    ("group 256 12,8,108 40,24,8 4096 5 r0r1r2",
     "matvec_kernel<12,5,true> m=0:40 n0=0 grid=10 block=256 lds=22080 arg=0; matvec_kernel<8,5,true> m=1:24 n0=0 grid=6 block=256 lds=23040 arg=0; "
     "matvec_kernel<108,5,true> m=2:8 n0=0 grid=2 block=256 lds=23040 arg=0"),
    ("group 256 13,14,12 40,24,8 1024 2 n MV_ONEPASS=0",
     "matvec_kmix_kernel<2,true> m=0:40,1:64,2:72 n0=0 grid=18 block=256 lds=10528 arg=256"),
    ("group 256 12,12,12 40,24,8 4096 7 n",
     "refused -5: qmm_mul_mat_group_ex: 7 rows of 4096 do not fit LDS with the norm"),
    ("group 256 12,12,12 40,24,8 5120 6 n",
     "refused -5: qmm_mul_mat_group_ex: 6 rows of 5120 do not fit LDS with the norm"),
    ("group 256 12,12 24,40 1024 1 s1",
     "refused -5: qmm_mul_mat_group_ex: swiglu wants two matrices of one type and shape, no residuals, all tokens in one launch"),
    ("group 256 12,12 24,24 1024 1 s1r0",
     "refused -5: qmm_mul_mat_group_ex: swiglu wants two matrices of one type and shape, no residuals, all tokens in one launch"),
]


def test_hand_pins_are_cases_of_the_table_and_hold(mv_plan_probe):  # noqa: F811
    specs = {F.probe_spec(c): c for _, c in ALL}
    got = mv_plan_probe([spec for spec, _ in HAND_PINS])
    for (spec, want), line in zip(HAND_PINS, got):
        assert spec in specs, spec
        assert line == want, spec
        case = specs[spec]
        assert (want.endswith(case.refusal) and want.startswith("refused -5: ")) if case.refusal else F.probe_line(case) == want, spec


def test_every_case_has_the_plan_the_header_gives(mv_plan_probe):  # noqa: F811
    """labels, matrices, first token of every sub-batch, block size, grid, LDS bytes, the one-pass bit and the refusals of every case: the plan
    header's own output equals the table's (matvec_fold_cases.plan, the header's rules restated in Python)"""
    cases = list({F.probe_spec(c): c for _, c in ALL}.values())
    assert len(cases) >= 1000
    got = mv_plan_probe([F.probe_spec(c) for c in cases])
    assert len(got) == len(cases)
    for c, line in zip(cases, got):
        if c.refusal:
            assert line.startswith("refused -5: ") and line.endswith(c.refusal) and not c.launches, (F.probe_spec(c), line)
        else:
            assert line == F.probe_line(c), F.probe_spec(c)
            assert all(l.lds <= F.LDS_LAUNCH for l in c.launches)


def test_named_plans_of_the_issue():
    """the decisions the table is built around, by name"""
    by = {(k, c.name): c for k, c in ALL}
    for n in (1, 4):
        assert F.labels_of(by[None, f"q80-res-4096-{n}"]) == (f"matvec_kmix_kernel<{n},true,q8_0>",)
        assert F.labels_of(by[None, f"q80-norm-4096-{n}"]) == (f"matvec_kernel<12,{n},true>", f"matvec_kernel<8,{n},true>", f"matvec_kernel<108,{n},true>")
    assert F.labels_of(by[None, "q80-res-4096-5"]) == ("matvec_kernel<12,5,true>", "matvec_kernel<8,5,true>", "matvec_kernel<108,5,true>")
    for t in F.REPS.values():
        a, b = by[t, "subbatch-16384-8"], by[t, "subbatch-28672-7"]
        assert F.labels_of(a) == (f"matvec_kernel<{t},4,true>",) * 2 and [l.n0 for l in a.launches] == [0, 4]
        assert F.labels_of(b) == (f"matvec_kernel<{t},4,true>", f"matvec_kernel<{t},3,true>") and [l.n0 for l in b.launches] == [0, 4]
    assert by[F.MIXED, "geo-norm-4096-6-2304"].launches[0][:2] == ("kmix", F.Q5_K) and by[F.MIXED, "geo-norm-4096-6-2304"].launches[0].waves == 16
    # the largest token counts the fit estimates take, and the first they refuse
    assert F.fits_norm(6, 4096) and not F.fits_norm(7, 4096) and F.fits_norm(5, 5120) and not F.fits_norm(6, 5120)
    assert F.fits_swiglu(6, 4096, True) and not F.fits_swiglu(7, 4096, True) and F.fits_norm(4, 6144) and not F.fits_norm(5, 6144)
    assert [c.refusal for c in F.cases_g()] == [F.REFUSE_NORM, F.REFUSE_NORM, F.REFUSE_SWIGLU, F.REFUSE_SWIGLU]


# ---- coverage, asserted from the table

def launches_of(t):
    """(case, launch) of every launch of weight type code t in the table (a mixed launch counts for each of its matrices' types)"""
    out = []
    for _, c in ALL:
        for l in c.launches:
            if t in [c.types[i] for i in l.idx]:
                out.append((c, l))
    return out


def test_the_table_has_all_23_type_codes():
    assert len(F.TYPES) == 23 and len(set(F.TYPES)) == 23 and len(F.WIRE) == 20
    assert sorted(t for ts in F.FAMILIES.values() for t in ts) == sorted(F.TYPES)
    assert all(F.family(t) == f for f, t in F.REPS.items())
    for f, a in (("F1", F.Q8_K), ("F2", F.Q8_K), ("F3", F.Q8_K), ("F4", 8), ("F5", F.Q8_1)):
        assert {F.act(t) for t in F.FAMILIES[f]} == {a}
    assert {F.bsg(t) for t in F.FAMILIES["F1"]} == {32} and {F.bsg(t) for t in F.FAMILIES["F2"] + F.FAMILIES["F3"]} == {16}


@pytest.mark.parametrize("t", F.TYPES, ids=[F.NAMES[t] for t in F.TYPES])
def test_every_type_has_every_fold_token_count_and_path(t):
    own = [(c, l) for c, l in launches_of(t) if l.kind == "type" and l.type == t]
    assert all(l.ex for _, l in own)
    assert {l.ntok for _, l in own} >= set(range(1, 9)), "an EX launch at every N in 1..8"
    assert any(c.norm and c.path == "two_step" for c, _ in own)
    assert any(c.res and not c.norm for c, _ in own) and any(c.res and c.form == "inplace" for c, _ in own)
    assert any(c.res == (1,) and len(c.types) == 3 for c, _ in own), "a residual on the second matrix only"
    assert {c.swiglu for c, _ in own} >= {1, 2} and any(c.swiglu and c.norm for c, _ in own) and any(c.swiglu and not c.norm for c, _ in own)
    if F.act(t) == F.Q8_K:
        one = {c.K for c, _ in own if c.norm and c.path == "one_pass" and not c.swiglu}
        assert one >= ({2048, 4096} if t == F.Q6_KP else {1024, 4096})
        assert any(c.ctx == "onepass=0" and c.path == "two_step" and c.K == 4096 for c, _ in own)
    else:
        assert not any(c.path == "one_pass" for c, _ in own)
    # the largest token counts the estimates take
    assert any(c.norm and not c.swiglu and (c.K, l.ntok) == (4096, 6) for c, l in own) and any(c.norm and c.swiglu and (c.K, l.ntok) == (4096, 6) for c, l in own)
    assert any(c.norm and (c.K, l.ntok) == ((6144, 4) if t == F.Q6_KP else (5120, 5)) for c, l in own)
    if not F.planar(t) and F.S.BLCK[t] == 32:
        assert any(c.norm and c.K == 1056 for c, _ in own), "33 blocks of 32"


@pytest.mark.parametrize("f", list(F.FAMILIES))
def test_every_family_has_every_geometry_and_sub_batches(f):
    own = [(c, l) for t in F.FAMILIES[f] for c, l in launches_of(t) if l.kind == "type"]
    for fold in (lambda c: c.norm and not c.swiglu, lambda c: c.norm and c.swiglu, lambda c: bool(c.res)):
        assert {l.waves for c, l in own if fold(c)} == {4, 8, 16}
    assert {(l.n0, l.ntok) for c, l in own if c.section == "e"} == {(0, 4), (4, 4), (4, 3)}
    assert any(c.section == "f" for c, _ in own)


def test_the_mixed_launches_have_every_fold_and_geometry():
    kmix = [(c, l) for _, c in ALL for l in c.launches if l.kind == "kmix"]
    assert all(l.ex for _, l in kmix)
    assert {(c.path, c.K) for c, _ in kmix if c.norm} >= {("one_pass", 1024), ("one_pass", 4096), ("two_step", 768), ("two_step", 5120)}
    assert {l.ntok for c, l in kmix if c.norm} >= {1, 3, 6} and {l.waves for c, l in kmix if c.norm} == {4, 8, 16} == {l.waves for c, l in kmix if c.res}
    assert any(c.res == (0, 1, 2) for c, _ in kmix) and any(c.res == (1,) for c, _ in kmix)
    assert any(F.Q6_KP in c.types for c, _ in kmix) and any(c.types[0] == F.Q6_K for c, _ in kmix)
    assert any(c.ctx == "onepass=0" for c, _ in kmix)
    q80 = [(c, l) for _, c in ALL for l in c.launches if l.kind == "kmix80"]
    assert {l.ntok for _, l in q80} == {1, 4} and all(l.ex and c.res for c, l in q80)


def test_declared_staging_paths_are_the_kernels_rule():
    """a case declares its path (written out per K in the table); the rule of matvec_kernel / matvec_kmix_kernel, restated: one pass <=> Q8_K
    activations, a norm, K <= 4096, K % 1024 == 0, the switch on"""
    seen = set()
    for _, c in ALL:
        assert c.path == F.rule_path(c), (c.name, c.types, c.K)
        seen.add(c.path)
    assert seen >= {"plain", "one_pass", "two_step", "refused"}


def test_shapes_stay_small():
    """the issue's limits: the largest weight buffer is 2304 rows of K = 5120, the largest K is 28672 on 8 rows"""
    for _, c in ALL:
        assert max(c.Ms) <= 2304 and c.K <= 28672 and (c.K <= 5120 or max(c.Ms) <= 72), c.name
        assert max(c.Ms) * c.K <= 2304 * 5120


# ---- the LDS invariant

def test_whatever_a_fit_estimate_accepts_fits_the_launch(mv_plan_probe):  # noqa: F811
    """the compiled sweep of the probe: every type, 1..8 tokens, K in block multiples to 32768; what mv_fits_plain / _norm / _swiglu / _mixed /
    _mixed_q80 accept asks for no more than MV_LDS_LAUNCH"""
    line, = mv_plan_probe(["sweep " + ",".join(map(str, F.TYPES))])
    print(line)
    assert line.startswith("sweep ok: "), line
    assert int(line.split()[2]) > 100000


# ---- the rounding-stable rows

def stable_shapes():
    """(activation format, K) of every launch with a norm in the table"""
    return sorted({(F.act(l.type), c.K) for _, c in ALL if c.norm for l in c.launches})


WEIGHT_OF = {H.Q8_K: F.Q4_K, H.Q8_0: F.Q4_0, H.Q8_1: F.Q4_1}     # a weight type the oracle dots against each activation format


def test_stable_shapes_are_the_tables():
    got = stable_shapes()
    assert {k for a, k in got if a == H.Q8_K} == {768, 1024, 2048, 4096, 5120, 6144}
    assert {k for a, k in got if a == H.Q8_0} == {k for a, k in got if a == H.Q8_1} == {768, 1024, 1056, 4096, 5120}


@pytest.mark.parametrize("fmt,k", stable_shapes(), ids=[f"{ {15: 'q8_K', 8: 'q8_0', 9: 'q8_1'}[a]}-{k}" for a, k in stable_shapes()])
def test_rounding_stable_rows(oracle, fmt, k):
    """the helper's own quantization is the oracle's byte for byte, and the oracle's bytes do not move when every element of the normed row is
    scaled by its own factor in 1 +- 2^-21 (far more than two f32 evaluations of the norm differ by).  Q8_K's d is an f32, 1 / (-127 / max):
    it follows the maximum by construction (to 2^-20 here) and is left out of the byte comparison of the perturbed rows"""
    n, eps = 8, 1e-5
    rng = np.random.default_rng(k + fmt)
    w = rng.normal(1, 0.1, k).astype(np.float32)
    x, redraws = H.rounding_stable_rows(fmt, n, k, w, eps, seed=fmt * 100000 + k)
    print(f"stable rows | format {fmt} K={k} | redraws per row: mean {redraws.mean():.2f} max {redraws.max()} (cap {H.STABLE_MAX_REDRAWS})")
    assert redraws.max() < H.STABLE_MAX_REDRAWS
    xn = H.rms_norm_f32(x, w, eps)
    want = oracle.quantize_act(WEIGHT_OF[fmt], xn)
    assert np.array_equal(H.quantize_stable(fmt, xn), want)
    size = 292 if fmt == H.Q8_K else 34 if fmt == H.Q8_0 else 36
    for trial in range(8):
        moved = (xn.astype(np.float64) * (1.0 + rng.uniform(-1, 1, xn.shape) * 2.0 ** -21)).astype(np.float32)
        assert not np.array_equal(moved, xn)
        got = oracle.quantize_act(WEIGHT_OF[fmt], moved).reshape(n, -1, size)
        ref = want.reshape(n, -1, size)
        if fmt == H.Q8_K:
            assert np.array_equal(got[:, :, 4:], ref[:, :, 4:])
            d0, d1 = ref[:, :, :4].copy().view(np.float32), got[:, :, :4].copy().view(np.float32)
            assert np.all(np.abs(d1 - d0) <= np.abs(d0) * 2.0 ** -20)
        else:
            assert np.array_equal(got, ref), (trial, np.argwhere(got != ref)[:4].tolist())


def test_unstable_rows_are_rejected():
    """the conditions bite: a row with an element on a half-integer step, a block scale on an f16 boundary, an all-zero block"""
    k = 256
    row = np.linspace(0.1, 1.0, k)
    row[-1] = 127.0
    assert H.rounding_stable(H.Q8_K, np.where(np.arange(k) == 3, 12.25, row))
    assert not H.rounding_stable(H.Q8_K, np.where(np.arange(k) == 3, 12.5, row))
    assert not H.rounding_stable(H.Q8_K, np.where(np.arange(k) == 3, -127.0, row)), "two maxima of opposite sign"
    blk = np.full(32, 0.25)
    d_mid = (float(np.float16(1.0)) + float(np.nextafter(np.float16(1.0), np.float16(2.0)))) / 2      # halfway between two f16 values
    assert H.rounding_stable(H.Q8_0, np.where(np.arange(32) == 0, 127.0, blk))
    assert not H.rounding_stable(H.Q8_0, np.where(np.arange(32) == 0, 127.0 * d_mid, blk * d_mid))
    assert not H.rounding_stable(H.Q8_0, np.concatenate([np.zeros(32), np.where(np.arange(32) == 0, 127.0, blk)]))
    with pytest.raises(RuntimeError):
        H.rounding_stable_rows(H.Q8_0, 1, 64, np.concatenate([np.zeros(32), np.ones(32)]).astype(np.float32), 1e-5)
