"""The MUL_MAT_ID case table: routing patterns and shape cases, shared by test_moe_routing_host.py (which pins the launch plan of
every case with a host probe on qmm_prefill_plan.h / qmm_matvec_plan.h) and test_gpu_moe_routing.py (which runs the cases and asserts
the traced labels equal the pins).  Plain Python and numpy.

A routing pattern is a function (n_tokens, n_used, n_expert, rng) -> ids int32 [n_tokens, n_used] that asserts its own post-condition
on np.bincount(ids), so that no test silently runs another distribution than the one it names.

The shape cases are the smallest at which each gathered kernel variant exists on a 256-CU device with the default switches
(P = n_tokens * n_used (token, slot) pairs)."""
from collections import namedtuple

import numpy as np

from oracle.pyoracle import IQ4_XS, Q2_K, Q3_K, Q4_1, Q4_K, Q5_1, Q5_K, Q6_K, Q8_K, vec_dot_type

CUS = 256                                    # the device the pins are written for
WIDE_UNITS = (Q6_K, Q2_K, Q3_K)              # types whose kernels step K by 128 (mfma_bk); every other type by 64


def k_values(t):
    """K per type.  32-weight blocks: 736 = 23 blocks (Kp = 768 is padded, so ksrc < K matters) and 1024.  256-weight blocks: 768 (12 K-steps
    over the 8 skinny waves: some waves get an empty range) and 1024 (the register-resident gathered prep, prep_act_q8k_kernel)."""
    return (768, 1024) if vec_dot_type(t) == Q8_K else (736, 1024)


# ------------------------------------------------------------------------------------------------------------- routing patterns

def _check(ids, n_tokens, n_used, n_expert):
    assert ids.dtype == np.int32 and ids.shape == (n_tokens, n_used) and ids.min() >= 0 and ids.max() < n_expert
    cnt = np.bincount(ids.ravel(), minlength=n_expert)
    assert cnt.sum() == n_tokens * n_used
    return cnt


def uniform(n_tokens, n_used, n_expert, rng):
    """the control: a per-token permutation of the experts, as the older tests route"""
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tokens)]).astype(np.int32)
    cnt = _check(ids, n_tokens, n_used, n_expert)
    assert cnt.max() <= n_tokens and all(len(set(r)) == n_used for r in ids.tolist())
    return ids


def one_hot(e):
    """every pair goes to expert e (negative: from the end); all slots of a token name the same expert"""
    def gen(n_tokens, n_used, n_expert, rng):
        ee = e % n_expert
        ids = np.full((n_tokens, n_used), ee, np.int32)
        cnt = _check(ids, n_tokens, n_used, n_expert)
        assert cnt[ee] == n_tokens * n_used and np.count_nonzero(cnt) == 1
        return ids
    gen.__name__ = f"one_hot({e})"
    return gen


def edge(c):
    """exactly c pairs (at random places) go to one middle expert, the others alternate over the first and the last expert; every
    other expert stays empty"""
    def gen(n_tokens, n_used, n_expert, rng):
        P = n_tokens * n_used
        assert n_expert >= 3 and 0 < c <= P
        mid, others = n_expert // 2, (0, n_expert - 1)
        where = rng.permutation(P)
        flat = np.empty(P, np.int32)
        flat[where[:c]] = mid
        flat[where[c:]] = np.where(np.arange(P - c) % 2 == 0, others[0], others[1])
        ids = flat.reshape(n_tokens, n_used)
        cnt = _check(ids, n_tokens, n_used, n_expert)
        assert cnt[mid] == c and cnt[others[0]] == (P - c + 1) // 2 and cnt[others[1]] == (P - c) // 2
        assert np.count_nonzero(cnt) == 1 + (P - c >= 1) + (P - c >= 2)
        return ids
    gen.__name__ = f"edge({c})"
    return gen


def sparse(n_tokens, n_used, n_expert, rng):
    """each token picks its experts from one random half of the experts: at least half of them receive nothing"""
    pool = rng.permutation(n_expert)[:n_expert // 2]
    assert n_used <= len(pool)
    ids = np.stack([rng.permutation(pool)[:n_used] for _ in range(n_tokens)]).astype(np.int32)
    cnt = _check(ids, n_tokens, n_used, n_expert)
    assert np.count_nonzero(cnt == 0) * 2 >= n_expert
    return ids


# ------------------------------------------------------------------------------------------------------------- shape cases

# kernel: (kind, a, b) for the types on 64-wide units, kernel_wide: for Q6_K / Q2_K / Q3_K (None: the same)
#   ("skinny", 8, NA)  mfma_skinny_kernel<t,8,NA>    token tile 32 * NA, fragment-major operand
#   ("regb", NW, BN)   mfma_regb_kernel<t,NW,BN>     token tile BN, NW * 32 rows
#   ("lds", TA, 128)   mfma_kernel<t,TA>             token tile 128, TA rows
# grid: the launch grid of that kernel, written out (grid_wide: of kernel_wide)
Case = namedtuple("Case", "name M n_expert n_tokens n_used kernel grid kernel_wide grid_wide")


def _c(name, M, n_expert, n_tokens, n_used, kernel, grid, kernel_wide=None, grid_wide=None):
    return Case(name, M, n_expert, n_tokens, n_used, kernel, grid, kernel_wide or kernel, grid_wide or grid)


DEFAULT_CASES = (
    _c("skinny-1",       96,  8,  10, 2, ("skinny", 8, 1), (3, 1, 8)),
    _c("skinny-2-p60",   96,  8,  30, 2, ("skinny", 8, 2), (3, 1, 8)),
    _c("skinny-2-p100",  96,  8,  50, 2, ("skinny", 8, 2), (3, 2, 8)),
    _c("regb-64-few",    320, 32, 50, 2, ("regb", 4, 64), (3, 2, 32)),         # P <= 128, but 10 row groups x 32 experts > 256 CUs: skinny declines
    _c("regb-32",        128, 4,  65, 2, ("regb", 4, 32), (1, 8, 4)),
    _c("regb-64",        512, 8,  129, 2, ("regb", 4, 64), (4, 6, 8)),
    _c("regb-128",       384, 32, 129, 2, ("regb", 4, 128), (3, 3, 32), ("regb", 4, 64), (3, 6, 32)),
    _c("regb-256",       256, 64, 100, 4, ("regb", 8, 128), (1, 4, 64)),
    _c("one-expert",     200, 1,  150, 1, ("regb", 4, 32), (2, 8, 1)),
    _c("sparse",         96,  64, 5,  6, ("skinny", 8, 1), (3, 1, 64)),
)
# QMM_PREC_BF16 (every type), and Q2_K / Q3_K with GGML_MI355X_REGB_Q23=0 in the default precision: the LDS-tile kernel with segments
LDS_CASES = (
    _c("lds-64",         96,  8,  30, 2, ("lds", 64, 128), (2, 1, 8)),
    _c("lds-128",        512, 16, 100, 4, ("lds", 128, 128), (4, 4, 16)),
)
BAD_ID_CASE = DEFAULT_CASES[5]               # P = 258


def pairs(case):
    return case.n_tokens * case.n_used


def kernel_of(case, t):
    return case.kernel_wide if t in WIDE_UNITS else case.kernel


def bn_of(case, t):
    """token extent of the case's tile"""
    kind, a, b = kernel_of(case, t)
    return 32 * b if kind == "skinny" else b


def label_of(case, t):
    kind, a, b = kernel_of(case, t)
    return {"skinny": f"mfma_skinny_kernel<{t},{a},{b}>", "regb": f"mfma_regb_kernel<{t},{a},{b}>", "lds": f"mfma_kernel<{t},{a}>"}[kind]


def grid_of(case, t):
    return case.grid_wide if t in WIDE_UNITS else case.grid


def prep_label_of(case, t, k, f16=True, regb_q23=True):
    """the activation prep: in registers for Q8_K activations of K % 1024 == 0 rows in the default precision (not IQ4_XS), else by LDS"""
    q8k = vec_dot_type(t) == Q8_K
    if q8k and f16 and k % 1024 == 0 and t != IQ4_XS:
        perm = 2 if t in (Q4_K, Q5_K) else 3 if t == Q6_K or regb_q23 else 0
        return f"prep_act_q8k_kernel<{perm}>"
    return f"prep_act_kernel<{15 if q8k else 8}>"


def labels_of(case, t, k, f16=True, regb_q23=True):
    """the launches of one prompt-batch MUL_MAT_ID call, in order: sort, prep, MFMA; for Q4_1 / Q5_1 in the default precision the deltas of
    the Q8_1 block sums in front of the MFMA launch and behind it the launch that adds the CPU's f16 rounding of those sums"""
    fix = f16 and t in (Q4_1, Q5_1)
    return ("moe_sort_kernel", prep_label_of(case, t, k, f16, regb_q23)) + (("moe_q81_delta_kernel",) if fix else ()) + (label_of(case, t),) + \
           ((f"moe_q81_sum_fix_kernel<{t}>",) if fix else ())


def pair_labels_of(case, t, k):
    """... of one mul_mat_id_pair call: one sort, one prep, one set of deltas; an MFMA launch (and a correction) per tensor"""
    one = labels_of(case, t, k)
    n = 3 if t in (Q4_1, Q5_1) else 2
    return one + one[n:]


def edge_counts(case, t):
    """segment lengths of the middle expert around the tile edge: BN - 1, BN, BN + 1 and 2 BN + 1 where the case has that many pairs; a
    case with fewer pairs than its tile takes P - 3"""
    bn, P = bn_of(case, t), pairs(case)
    return tuple(c for c in (bn - 1, bn, bn + 1, 2 * bn + 1) if c <= P) or (P - 3,)


def patterns(case, t):
    """the (name, generator) list of a case: the control, one-hot at both ends, the tile edges, sparse where the case is made for it"""
    if case.name == "sparse":
        return (("sparse", sparse),)
    out = [("uniform", uniform), ("one_hot(0)", one_hot(0)), ("one_hot(-1)", one_hot(-1))]
    if case.n_expert >= 3:
        out += [(f"edge({c})", edge(c)) for c in edge_counts(case, t)]
    return tuple(out)


def make_ids(case, t, name, gen):
    """the ids of (case, pattern): seeded by the names alone, so that the host test and every GPU test see the same routing"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name + name))
    return gen(case.n_tokens, case.n_used, case.n_expert, np.random.default_rng(seed))


# ------------------------------------------------------------------------------------------------------------- few-pair cases

# matvec_id_kernel / matvec_id_swiglu_kernel past one wave of units: K = 4352 is 68 units of 64 or 136 units of 32 (the second slice
# runs, partially filled); M = 41 is ragged against the 8 waves.  M = 300 at 16 pairs: the plan caps grid[1], the row loop runs again.
# 136 units are two slices and a third of 8 lanes; the 64-wide units get theirs at K = 8448 (132 units), on the first two cases.
FEW_K = 4352
FEW_K_LONG = 8448


def mv_unit_width(t):
    """weights per mat-vec unit (MvUnit<T>::W): a lane of a wave takes one unit per slice"""
    return 64 if t in (Q4_K, Q5_K, Q6_K, Q2_K, Q3_K) else 32


# grid_y: grid[1] of the single, the pair and the SwiGLU launch, written out (6 chunks of 8 rows cover M = 41; 300 rows want 38 chunks,
# the plan caps them so that the launch has about two workgroups per CU)
FewCase = namedtuple("FewCase", "M n_tokens n_used n_expert pattern grid_y")
FEW_CASES = (
    FewCase(41, 1, 2, 8, "uniform", (6, 6, 6)),
    FewCase(41, 8, 2, 8, "uniform", (6, 6, 6)),
    FewCase(41, 2, 6, 8, "uniform", (6, 6, 6)),
    FewCase(41, 8, 2, 8, "one_hot(-1)", (6, 6, 6)),
    FewCase(300, 8, 2, 4, "one_hot(0)", (32, 16, 32)),
)
FEW_PATTERNS = {"uniform": uniform, "one_hot(-1)": one_hot(-1), "one_hot(0)": one_hot(0)}


def few_k_cases(t):
    """(K, case) of the few-pair test: every case at FEW_K, and for the 64-wide units the first two again at FEW_K_LONG"""
    return [(FEW_K, fc) for fc in FEW_CASES] + ([(FEW_K_LONG, fc) for fc in FEW_CASES[:2]] if mv_unit_width(t) == 64 else [])


def few_ids(fc):
    seed = fc.M * 1000 + fc.n_tokens * 10 + fc.n_used
    return FEW_PATTERNS[fc.pattern](fc.n_tokens, fc.n_used, fc.n_expert, np.random.default_rng(seed))
