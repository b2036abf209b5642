"""The plain MUL_MAT prefill case table: every branch of prefill_plan (csrc/qmm_prefill_plan.h) a prompt batch can take without gather, and
every class of split-K range the tiled kernels cut K into.  Shared by test_mulmat_plan_host.py (which pins the launch plan of every case with a
host probe on the plan header) and test_gpu_mulmat_branches.py (which runs the cases against two CPU references, per token row and per weight
row, and asserts the traced labels equal the pins).  Plain Python and numpy.

The pins are written for a 256-CU device with the default switches; a case that needs another context names it (CONTEXTS).  M = weight rows,
N = tokens, the output is [N, M].  The shapes are the smallest at which each branch exists on such a device.

Split-K ranges.  The tiled kernels cut K into `ksplit` ranges, one workgroup (blockIdx.z) each:
  * mfma_regb_kernel (qmm_mfma_regb.hiph, `const int per = ((nk + ksplit - 1) / ksplit + 1) & ~1` and the line behind it): K-steps of BK
    weights, nk = Kp / BK of the padded row, an even count per range;
  * the Q4_K kernels (mfma_regb_q4k_kernel, mfma_regb_q4k_wide_kernel and mfma_r64_q4k_kernel in the same file, `const int bper = (nblk +
    ksplit - 1) / ksplit`; mfma_r64s_q4k_kernel in qmm_mfma_r64s.hiph): whole 256-weight blocks, nblk = K / 256.
Range `split` is [split * per, min(split * per + per, n)): the rounding up can leave the last range shorter (ragged), empty, or beginning
past the end of K (a negative length: the loop does not run, the loads are clamped, the slab must still be written as zeros and, with the
in-launch combine, the arrival counter still bumped).  range_lengths() restates the two formulas; the table writes the lengths out."""
from collections import namedtuple

from oracle.pyoracle import IQ4_XS, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, Q8_K, vec_dot_type

CUS = 256                                    # the device the pins are written for
MAX_OUT = 16 << 20                           # no case's output has more elements
WIDE_UNITS = (Q6_K, Q2_K, Q3_K)              # types whose kernels step K by 128 (mfma_bk); every other type by 64

# name -> (environment read when a context is created, the same as switches of the host probe, QMM_PREC_BF16)
CONTEXTS = {
    "default": ({}, "", False),
    "bf16":    ({}, "", True),
    "combine": ({"GGML_MI355X_SPLITK_COMBINE": "1"}, "SPLITK_COMBINE=1", False),
    "r64=1":   ({"GGML_MI355X_R64": "1"}, "R64=1", False),
    "r64=0":   ({"GGML_MI355X_R64": "0"}, "R64=0", False),
    "r64s=0":  ({"GGML_MI355X_R64S": "0"}, "R64S=0", False),
}


def family(t):
    """b32: blocks of 32 weights (K any multiple of 32, Kp padded to 128); b64: 256-weight blocks walked in 64-wide K-steps (Q5_K, IQ4_XS);
    b128: ... in 128-wide K-steps; q4k: the Q4_K kernels, which walk whole blocks"""
    return "q4k" if t == Q4_K else "b128" if t in WIDE_UNITS else "b64" if vec_dot_type(t) == Q8_K else "b32"


def bk(t):
    return 128 if t in WIDE_UNITS else 64


def kpad(k):
    return (k + 127) // 128 * 128


def range_lengths(t, k, ksplit):
    """lengths of the K ranges of a split-K launch, in the kernel's own unit (K-steps of bk(t), or Q4_K blocks); the formulas of the module
    docstring restated"""
    if t == Q4_K:
        n, per = k // 256, (k // 256 + ksplit - 1) // ksplit
    else:
        n = kpad(k) // bk(t)
        per = ((n + ksplit - 1) // ksplit + 1) & ~1
    return tuple(min(s * per + per, n) - s * per for s in range(ksplit))


def range_class(lengths):
    """even: every range the same; ragged: a shorter last one; empty: a range of no steps; past-end: a range that begins beyond K"""
    if lengths is None:
        return None
    if min(lengths) < 0:
        return "past-end"
    if min(lengths) == 0:
        return "empty"
    return "even" if len(set(lengths)) == 1 else "ragged"


# ------------------------------------------------------------------------------------------------------------- the cases

# kernel: (kind, a, b)
#   ("regb", NW, BN)   mfma_regb_kernel<t,NW,BN>     32 * NW rows x BN tokens (Q4_K: mfma_regb_q4k_kernel under the same label)
#   ("skinny", 8, NA)  mfma_skinny_kernel<t,8,NA>    token tile 32 * NA, fragment-major operand
#   ("lds", TA, 0)     mfma_kernel<t,TA>             TA rows x 128 tokens
#   ("wide", 8, 0) mfma_regb_q4k_wide_kernel<8>, ("r64", 4 | 8, 0) mfma_r64_q4k_kernel<4 | 8>, ("r64s", 2, 0) mfma_r64s_q4k_kernel<2>
# A launch covers matrices first .. first + n - 1 of the call; prep: the activation prep runs in front of it; reduce: splitk_reduce_kernel
# behind it; combine: the launch adds the ranges itself (label + "+combine", no reduce kernel); wide: 256-token tiles
Launch = namedtuple("Launch", "first n prep kernel grid ksplit reduce combine wide")
# Ms: rows of the 1..4 matrices; ranges: the range lengths of the case's split-K launch, written out (None: ksplit == 1); repeat: how
# often the call runs, each time into re-filled outputs; section: the part of the table (a .. g as the GPU tests name them, w: the 256-token tiles of f)
Case = namedtuple("Case", "name section ctx Ms K N launches ranges repeat")


def _l(kernel, grid, ksplit=1, first=0, n=1, prep=True, combine=False, wide=False):
    return Launch(first, n, prep, kernel, grid, ksplit, ksplit > 1 and not combine, combine, wide)


def _c(name, section, ctx, Ms, K, N, launches, ranges=None, repeat=1):
    Ms = Ms if isinstance(Ms, tuple) else (Ms,)
    launches = (launches,) if isinstance(launches, Launch) else launches
    return Case(name, section, ctx, Ms, K, N, launches, ranges, repeat)


R8 = ("regb", 8, 128)
# split-K on the 256 x 128 tile, M = 300 (two row tiles, the second ragged; M % 4 == 0: the float4 reduce) x N = 129 (two token tiles, the
# second of one token): family -> ((K, ksplit, range lengths), ...).
SPLITK = {
    "b32": ((1056, 2, (10, 8)), (2336, 4, (10, 10, 10, 8)), (2592, 5, (10, 10, 10, 10, 2)), (4160, 8, (10, 10, 10, 10, 10, 10, 6, -4)),
            (4480, 8, (10, 10, 10, 10, 10, 10, 10, 0))),
    "b64": ((1024, 2, (8, 8)), (1280, 2, (10, 10)), (2048, 4, (8, 8, 8, 8)), (2304, 4, (10, 10, 10, 6)), (2816, 5, (10, 10, 10, 10, 4)),
            (3840, 7, (10, 10, 10, 10, 10, 10, 0)), (4352, 8, (10, 10, 10, 10, 10, 10, 8, -2))),
    "b128": ((1024, 2, (4, 4)), (1280, 2, (6, 4)), (2048, 4, (4, 4, 4, 4)), (2304, 4, (6, 6, 6, 0)), (2816, 5, (6, 6, 6, 4, -2)),
             (3840, 7, (6, 6, 6, 6, 6, 0, -6)), (4352, 8, (6, 6, 6, 6, 6, 4, -2, -8))),
    "q4k": ((1024, 2, (2, 2)), (1280, 2, (3, 2)), (2048, 4, (2, 2, 2, 2)), (2304, 4, (3, 3, 3, 0)), (2816, 5, (3, 3, 3, 2, -1)),
            (3840, 7, (3, 3, 3, 3, 3, 0, -3)), (4352, 8, (3, 3, 3, 3, 3, 2, -1, -4))),
}
# ... again at M = 253 (one ragged row tile, M % 4 != 0: the scalar reduce), at these K
SCALAR_REDUCE_K = {"b32": (4160, 4480), "b64": (3840, 4352), "b128": (2304, 4352), "q4k": (2304, 4352)}
# the 65..128-token band above the few-token kernel's row limit, the group launch and the in-launch combine: family -> (K, range lengths)
BAND = {"b32": (1056, (10, 8)), "b64": (1280, (10, 10)), "b128": (1280, (6, 4)), "q4k": (1280, (3, 2))}
FOUR = {"b32": (2336, (10, 10, 10, 8)), "b64": (2304, (10, 10, 10, 6)), "b128": (2304, (6, 6, 6, 0)), "q4k": (2304, (3, 3, 3, 0))}


def tile_k(t):
    """K of the ksplit == 1 cases: 23 blocks of 32 (Kp = 768 is padded: the clamped loads and zeroed scales past K count), or 3 of 256"""
    return 736 if family(t) == "b32" else 768


def cases(t):
    """every case of weight type t, in the order the GPU tests run them"""
    f, k0 = family(t), tile_k(t)
    out = [
        # a. tile variants, ksplit == 1
        _c("tile-4x32", "a", "default", 300, k0, 129, _l(("regb", 4, 32), (3, 8, 1))),
        _c("tile-4x64", "a", "default", 2048, k0, 512, _l(("regb", 4, 64), (16, 8, 1))),
        # 5 x 52 tiles of 128 x 128 fill 256 CUs; the 128-wide units have no such tile (it spills) and take 128 x 64 at half the tokens
        _c("tile-4x64-wide-units", "a", "default", 640, k0, 3328, _l(("regb", 4, 64), (5, 52, 1))) if f == "b128" else
        _c("tile-4x128", "a", "default", 640, k0, 6656, _l(("regb", 4, 128), (5, 52, 1))),
        # 100 tokens, but 257 row groups of 32 are more than the CUs: the few-token kernel declines
        _c("band-65-128", "a", "default", 8224, BAND[f][0], 100, _l(R8, (33, 1, 2), 2), BAND[f][1]),
        _c("skinny-32", "a", "default", 300, k0, 32, _l(("skinny", 8, 1), (10, 1, 1))),
        _c("skinny-64", "a", "default", 300, k0, 64, _l(("skinny", 8, 2), (10, 1, 1))),
        _c("skinny-128", "a", "default", 300, k0, 128, _l(("skinny", 8, 2), (10, 2, 1))),
    ]
    # b. the split-K range classes, c. both reduce paths
    out += [_c(f"splitk-{k}", "b", "default", 300, k, 129, _l(R8, (2, 2, s), s), r) for k, s, r in SPLITK[f]]
    out += [_c(f"splitk-{k}-scalar-reduce", "b", "default", 253, k, 129, _l(R8, (1, 2, s), s), r) for k, s, r in SPLITK[f] if k in SCALAR_REDUCE_K[f]]
    # d. groups: one launch over the row tiles of three matrices (2 + 1 + 2) and one reduce; two matrices too small for that, each alone
    kf, rf = FOUR[f]
    out += [
        _c("group-one-launch", "d", "default", (300, 70, 257), kf, 300, _l(R8, (5, 3, 4), 4, n=3), rf),
        _c("group-per-matrix", "d", "default", (300, 70), k0, 300, (_l(("regb", 4, 32), (3, 12, 1)), _l(("regb", 4, 32), (1, 12, 1), first=1, prep=False))),
    ]
    # e. GGML_MI355X_SPLITK_COMBINE=1: every M % 4 == 0; four times, so that the counters' return to zero counts (with an empty range)
    out += [
        _c("combine", "e", "combine", 304, kf, 129, _l(R8, (2, 2, 4), 4, combine=True), rf, repeat=4),
        _c("combine-group", "e", "combine", (300, 72, 256), kf, 300, _l(R8, (4, 3, 4), 4, n=3, combine=True), rf, repeat=4),
    ]
    # f. the Q4_K kernels behind switches
    if t == Q4_K:
        r4 = ("r64", 4, 0)
        out += [_c(f"r64-splitk-{k}", "f", "r64=1", 300, k, 129, _l(r4, (2, 2, s), s), r) for k, s, r in SPLITK[f]]
        out += [_c("r64-group-one-launch", "f", "r64=1", (300, 70, 257), kf, 300, _l(r4, (5, 3, 4), 4, n=3), rf)]
        # 256-token tiles: 28 x 8 of them (ragged rows: 7000 = 27 x 256 + 88, ragged tokens: 1950 = 7 x 256 + 158); two blocks of K
        for ctx, kernel in (("r64=0", ("wide", 8, 0)), ("default", ("r64s", 2, 0)), ("r64s=0", ("r64", 8, 0))):
            out += [_c(f"wide-{kernel[0]}{kernel[1]}", "w", ctx, 7000, 512, 1950, _l(kernel, (28, 8, 1), wide=True)),
                    _c(f"wide-pair-{kernel[0]}{kernel[1]}", "w", ctx, (3500, 3600), 512, 1950, _l(kernel, (29, 8, 1), n=2, wide=True))]
    # g. QMM_PREC_BF16: the LDS-tile kernel
    out += [
        _c("bf16-64", "g", "bf16", 300, k0, 129, _l(("lds", 64, 0), (5, 2, 1))),
        _c("bf16-128", "g", "bf16", 2048, k0, 2048, _l(("lds", 128, 0), (16, 16, 1))),
    ]
    return out


def label_of(launch, t):
    kind, a, b = launch.kernel
    text = {"regb": f"mfma_regb_kernel<{t},{a},{b}>", "skinny": f"mfma_skinny_kernel<{t},{a},{b}>", "lds": f"mfma_kernel<{t},{a}>",
            "wide": f"mfma_regb_q4k_wide_kernel<{a}>", "r64": f"mfma_r64_q4k_kernel<{a}>", "r64s": f"mfma_r64s_q4k_kernel<{a}>"}[kind]
    return text + ("+combine" if launch.combine else "")


def prep_label_of(case, t):
    """the activation prep: in registers for Q8_K activations of K % 1024 == 0 rows in the default precision (not IQ4_XS), else by LDS"""
    q8k = vec_dot_type(t) == Q8_K
    if q8k and case.ctx != "bf16" and case.K % 1024 == 0 and t != IQ4_XS:
        return f"prep_act_q8k_kernel<{2 if t in (Q4_K, Q5_K) else 3}>"
    return f"prep_act_kernel<{15 if q8k else 8}>"


def labels_of(case, t):
    """the launches of one call, in order: per launch the prep (where it runs), the MFMA kernel, the reduce (where it runs)"""
    out = []
    for l in case.launches:
        out += ([prep_label_of(case, t)] if l.prep else []) + [label_of(l, t)] + (["splitk_reduce_kernel"] if l.reduce else [])
    return tuple(out)


DIRTY_FACTOR = 8                             # >= the largest ksplit


def dirty_rows(case):
    """Rows of the launch that dirties the split-K workspace in front of a case whose ranges are empty or begin past the end (None: the case needs
    none).  Such a range must leave a slab of zeros; a kernel that skipped the store would hand the reduce whatever the workspace held, and
    whether that shows must not depend on which cases ran before.  One matrix of DIRTY_FACTOR x the case's rows at the same K and N, in the same
    context, is again a split-K launch with its slabs at the same offset (the offset depends on the padded N and K alone), and its slab 0, the
    partial sums of a range that has work, is as large as all DIRTY_FACTOR >= ksplit slabs of the case together (test_mulmat_plan_host.py pins
    this)"""
    return DIRTY_FACTOR * sum(case.Ms) if range_class(case.ranges) in ("empty", "past-end") else None


def out_elements(case):
    return case.N * sum(case.Ms)
