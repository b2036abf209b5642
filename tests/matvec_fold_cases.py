"""The case table of the few-token mat-vec folds (qmm_mul_mat_group_ex at N <= 8: the RMS norm folded into the activation staging, the
SwiGLU of a gate / up pair, the residual added in the epilogue) for every weight type code the library has, wire and planar.  Shared by
test_matvec_fold_host.py (which pins the launch plan of every case with the host probe on csrc/qmm_matvec_plan.h and asserts what the table
covers) and test_gpu_matvec_folds.py (which runs the cases against the CPU references and asserts the traced labels equal the pins).  Plain
Python and numpy.

The pins are for a 256-CU device with the default switches; the one other context is GGML_MI355X_MV_ONEPASS=0 (CONTEXTS).  M = weight rows,
N = tokens, the output is [N, M].

Families, by what the staging does with a type (csrc/qmm_matvec.hiph: stage_q8k_rows, quantize_rows, act_pos; csrc/qmm_mvunit.hiph):
  F1  Q8_K activations, block sums per 32, Q4_K's LDS order
  F2  Q8_K, sums per 16, Q6_K's order
  F3  Q8_K, the 32-weight sub-block order
  F4  Q8_0 activations (Q4_0P: Q4_K's order, a two-block unit)
  F5  Q8_1 activations
Staging paths: `plain` (no norm: quantize_rows from global memory), `one_pass` (norm and Q8_K quantization in registers, stage_q8k_rows:
Q8_K activations, K <= 4096, K % 1024 == 0, the switch on), `two_step` (stage_rms_norm into LDS, then quantize_rows).  A case DECLARES its
path (PATHS below, written out per K); test_matvec_fold_host.py compares the declaration with the kernel's rule.

plan() restates matvec_group_plan / matvec_launch / matvec_extras_check of the plan header in Python: the launches of a case (label, matrices,
first token, block size, grid, LDS bytes) are what that restatement gives, and the host test holds the header's own output (the probe of
test_host_logic.py) to it, besides pins written out by hand."""
from collections import namedtuple

from ggml_hexagon_amd import synth as S

CUS = 256
Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = S.Q4_0, S.Q4_1, S.Q5_0, S.Q5_1, S.Q8_0, S.Q2_K, S.Q3_K, S.Q4_K, S.Q5_K, S.Q6_K
IQ4_NL, IQ4_XS, IQ3_XXS, IQ3_S, IQ2_XS, IQ2_S, IQ1_S, IQ1_M, TQ1_0, TQ2_0 = (S.IQ4_NL, S.IQ4_XS, S.IQ3_XXS, S.IQ3_S, S.IQ2_XS, S.IQ2_S, S.IQ1_S,
                                                                             S.IQ1_M, S.TQ1_0, S.TQ2_0)
Q8_1, Q8_K = 9, 15                           # activation formats only
Q4_0P, Q8_0P, Q6_KP = 102, 108, 114          # the planar codes (qmm_repack_rows)
WIRE = tuple(S.NAMES)
TYPES = WIRE + (Q4_0P, Q8_0P, Q6_KP)
NAMES = {**S.NAMES, Q4_0P: "q4_0-planar", Q8_0P: "q8_0-planar", Q6_KP: "q6_K-planar"}
CODEBOOK_TYPES = (IQ3_XXS, IQ3_S, IQ2_XS, IQ2_S, IQ1_S, IQ1_M)      # grids handed over at run time (qmm_set_codebook)

FAMILIES = {
    "F1": (Q4_K, Q5_K),
    "F2": (Q6_K, Q6_KP, Q2_K, Q3_K, TQ2_0),
    "F3": (IQ4_XS, IQ3_XXS, IQ3_S, IQ2_XS, IQ2_S, IQ1_S, IQ1_M, TQ1_0),
    "F4": (Q4_0, Q5_0, Q8_0, IQ4_NL, Q8_0P, Q4_0P),
    "F5": (Q4_1, Q5_1),
}
REPS = {"F1": Q5_K, "F2": Q3_K, "F3": IQ4_XS, "F4": Q5_0, "F5": Q5_1}      # one type per family (sections c, e, f)
MIXED = "mixed"                                                             # the mixed K-quant group, where a table is keyed by type

# name -> (environment read when a context is created, the same as a switch of the host probe)
CONTEXTS = {"default": ({}, ""), "onepass=0": ({"GGML_MI355X_MV_ONEPASS": "0"}, "MV_ONEPASS=0")}

MV_MAX_N, MV_MAX_GROUP = 8, 4
LDS_LAUNCH, LDS_FIT = 160 * 1024, 150 * 1024


def base(t):
    return t - 100 if t >= 100 else t


def planar(t):
    return t >= 100


def family(t):
    return [f for f, ts in FAMILIES.items() if t in ts][0]


def act(t):
    """the activation format of a weight type (type_act)"""
    return Q8_K if S.BLCK[base(t)] == 256 else Q8_1 if base(t) in (Q4_1, Q5_1) else Q8_0


def k_ok(t, k):
    """K a type takes: a multiple of its block; planar rows 256 (Q6_KP: 2048)"""
    return k % (2048 if t == Q6_KP else 256 if planar(t) else S.BLCK[t]) == 0


# ------------------------------------------------------------------------------------------------- the header's rules, restated

def bsg(t):
    return 32 if base(t) in (Q4_K, Q5_K) else 16


def act_bytes(t, n, k):
    a = act(t)
    b = n * k + n * (k // (256 if a == Q8_K else 32)) * 4
    if a == Q8_K:
        b += n * (k // bsg(t)) * 2
    if a == Q8_1:
        b += n * (k // 32) * 4
    return (b + 15) & ~15


def kmix_act_bytes(n, k):
    return (n * k + n * (k // 256) * 4 + n * (k // 16) * 2 + 15) & ~15


def fits_plain(n, k):
    return n * k * 5 // 4 + 4096 <= LDS_FIT


def fits_norm(n, k):
    return n * k * 4 + n * k * 11 // 8 + 4096 <= LDS_FIT


def fits_swiglu(n, k, norm):
    return n * k * 5 // 4 + (n * k * 4 if norm else 0) + 4096 <= LDS_FIT


def fits_mixed(n, k):
    return n * k * 11 // 8 + 4096 <= LDS_FIT


def fits_mixed_q80(n, k):
    return n * k * 21 // 8 + 4096 <= LDS_FIT


def kernel_path(types, k, norm, onepass=True):
    """the staging path of a launch, as matvec_kernel / matvec_kmix_kernel decide it"""
    if not norm:
        return "plain"
    return "one_pass" if act(types[0]) == Q8_K and k <= 4096 and k % 1024 == 0 and onepass else "two_step"


def rule_path(case):
    """the staging path(s) the kernels take in the case's launches: one name, or the runs' names joined by "+" where they differ"""
    if case.refusal:
        return "refused"
    paths = [kernel_path((l.type,), case.K, case.norm, case.ctx == "default") for l in case.launches]
    return paths[0] if len(set(paths)) == 1 else "+".join(paths)


# kind: "type" matvec_kernel<t, ntok, ex>, "kmix" matvec_kmix_kernel<ntok, ex>, "kmix80" matvec_kmix_kernel<ntok, ex, q8_0>; idx: the matrices
# of the call it covers; rows: their cumulative row counts; n0 / ntok: its tokens; waves per workgroup, workgroups, LDS bytes; arg: the
# act_mode argument (256: the one-pass staging switched off)
Launch = namedtuple("Launch", "kind type idx rows n0 ntok ex waves grid lds arg")

REFUSE_NORM = "do not fit LDS with the norm"
REFUSE_SWIGLU = "swiglu wants two matrices of one type and shape, no residuals, all tokens in one launch"


def label(l):
    ex = "true" if l.ex else "false"
    return {"type": f"matvec_kernel<{l.type},{l.ntok},{ex}>", "kmix": f"matvec_kmix_kernel<{l.ntok},{ex}>",
            "kmix80": f"matvec_kmix_kernel<{l.ntok},{ex},q8_0>"}[l.kind]


def _launch(kind, types, Ms, idx, k, n0, ntok, norm, swiglu, res, onepass):
    rows, total = [], 0
    for i in idx:
        total += Ms[i]
        rows.append(total)
    ex = bool(norm or swiglu or any(i in res for i in idx))
    t = types[idx[0]]
    lds = (act_bytes(t, ntok, k) if kind == "type" else kmix_act_bytes(ntok, k)) + (ntok * k * 4 if norm else 0) + \
          (act_bytes(Q8_0P, ntok, k) if kind == "kmix80" else 0)
    assert lds <= LDS_LAUNCH and not (kind == "kmix80" and ntok > 4)
    total = rows[0] if kind == "type" and swiglu else rows[-1]
    per_cu = (total + CUS - 1) // CUS
    waves = 16 if per_cu > 8 else 8 if per_cu > 4 else 4
    return Launch(kind, t, tuple(idx), tuple(rows), n0, ntok, ex, waves, min((total + waves - 1) // waves, CUS), lds, 0 if onepass else 256)


def plan(types, Ms, k, n, norm=False, swiglu=0, res=(), onepass=True):
    """(launches, refusal): matvec_extras_check, then matvec_group_plan run by run, for the default rules (mv_kmix = 2, one block per CU)"""
    nw = len(types)
    assert n <= MV_MAX_N and nw <= MV_MAX_GROUP and all(m > 0 for m in Ms)
    if norm and not fits_norm(n, k):
        return (), REFUSE_NORM
    if swiglu and (nw != 2 or types[0] != types[1] or Ms[0] != Ms[1] or res or not fits_swiglu(n, k, norm)):
        return (), REFUSE_SWIGLU
    kq = lambda t: t in (Q4_K, Q5_K, Q6_K, Q6_KP)
    q80 = lambda t: t in (Q8_0, Q8_0P)
    if 2 <= nw and any(t != types[0] for t in types):
        n_k, n_80 = sum(kq(t) for t in types), sum(q80(t) for t in types)
        ok = n_k + n_80 == nw
        if n_80:
            ok = ok and n_k > 0 and n <= 4 and not norm and not swiglu and fits_mixed_q80(n, k)
        if ok and fits_mixed(n, k):
            return (_launch("kmix80" if n_80 else "kmix", types, Ms, range(nw), k, 0, n, norm, swiglu, res, onepass),), None
    out, first = [], 0
    while first < nw:
        nxt = first
        while nxt < nw and types[nxt] == types[first] and nxt - first < MV_MAX_GROUP:
            nxt += 1
        at_once = n
        while at_once > 1 and not fits_plain(at_once, k):
            at_once = (at_once + 1) // 2
        for n0 in range(0, n, at_once):
            out.append(_launch("type", types, Ms, range(first, nxt), k, n0, min(n - n0, at_once), norm, swiglu, res, onepass))
        first = nxt
    return tuple(out), None


# ------------------------------------------------------------------------------------------------- the cases

# types / Ms: the call's matrices; res: the matrices with a residual; form: "out" (dst and residual in buffers of their own) or "inplace"
# (dst is the residual buffer); path: the DECLARED staging path; launches / refusal: plan() of the call
Case = namedtuple("Case", "name section ctx types Ms K N norm swiglu res form path launches refusal")


def _c(name, section, types, Ms, k, n, path, norm=False, swiglu=0, res=(), form="out", ctx="default"):
    types, Ms = tuple(types), tuple(Ms)
    assert all(k_ok(t, k) for t in types), (name, k)
    launches, refusal = plan(types, Ms, k, n, norm, swiglu, tuple(res), onepass=ctx == "default")
    return Case(name, section, ctx, types, Ms, k, n, norm, swiglu, tuple(res), form, path, launches, refusal)


GROUP_MS = (40, 24, 8)                       # the first rows of one 4-wave workgroup's waves fall into different matrices
# the declared staging path of a norm launch on Q8_K activations, per K (every other activation format: two_step)
PATHS = {768: "two_step", 1024: "one_pass", 2048: "one_pass", 4096: "one_pass", 5120: "two_step", 6144: "two_step"}


def norm_path(t, k):
    return PATHS[k] if act(t) == Q8_K else "two_step"


def norm_shapes(t):
    """(K, token counts) of the norm launches of section a.  Q6_KP rows exist at K % 2048 == 0 only: 2048 stands for 1024 (one pass), 6144
    for 5120 and 768 (two steps: the nearest such K above 4096), with 4 tokens, the most mv_fits_norm takes there"""
    if t == Q6_KP:
        return ((2048, tuple(range(1, 9))), (4096, (1, 6)), (6144, (1, 4)))
    wire32 = not planar(t) and S.BLCK[t] == 32
    return ((1024, tuple(range(1, 9))), (4096, (1, 6)), (5120, (1, 5)), (768, (1, 8))) + (((1056, (1, 8)),) if wire32 else ())


def small_k(t):
    """the one-block K of the residual and SwiGLU launches"""
    return 2048 if t == Q6_KP else 256


def cases_a(t):
    """every fold at the smallest shapes"""
    out = []
    for k, ns in norm_shapes(t):
        for n in ns:
            out.append(_c(f"norm-{k}-{n}", "a-norm", (t,) * 3, GROUP_MS, k, n, "two_step" if k == 1056 else norm_path(t, k), norm=True))
    for k in (small_k(t), 4096):
        for n in (1, 4, 8):
            out.append(_c(f"res-{k}-{n}", "a-res", (t,), (40,), k, n, "plain", res=(0,)))
            out.append(_c(f"res-inplace-{k}-{n}", "a-res", (t,), (40,), k, n, "plain", res=(0,), form="inplace"))
            out.append(_c(f"res-second-{k}-{n}", "a-res", (t,) * 3, GROUP_MS, k, n, "plain", res=(1,)))
        for n in (1, 3, 8):
            for which in (1, 2):
                out.append(_c(f"swiglu{which}-{k}-{n}", "a-swiglu", (t,) * 2, (24, 24), k, n, "plain", swiglu=which))
    k1 = 2048 if t == Q6_KP else 1024
    for k, n in ((k1, 1), (k1, 3), (4096, 6)):
        for which in (1, 2):
            out.append(_c(f"swiglu{which}-norm-{k}-{n}", "a-swiglu", (t,) * 2, (24, 24), k, n, norm_path(t, k), norm=True, swiglu=which))
    return out


KMIX_GROUPS = (((Q5_K, Q6_K, Q4_K), (40, 24, 8)), ((Q6_K, Q5_K, Q4_K), (8, 40, 24)))      # in the second, wave 0's first row is no Q4_K row
Q80_GROUP = ((Q4_K, Q8_0, Q8_0P), (40, 24, 8))


def with_planar_q6k(types):
    return tuple(Q6_KP if t == Q6_K else t for t in types)


def cases_b():
    """mixed launches: matvec_kmix_kernel with every fold it takes"""
    out = []
    for g, (types, Ms) in enumerate(KMIX_GROUPS):
        for k in (1024, 4096, 768, 5120):
            variants = [("wire", types)] + ([("planar", with_planar_q6k(types))] if k % 2048 == 0 else [])
            for vname, ts in variants:
                for n in (1, 3, 6):
                    if fits_norm(n, k):
                        out.append(_c(f"kmix{g}-{vname}-norm-{k}-{n}", "b", ts, Ms, k, n, PATHS[k], norm=True))
                    if k in (1024, 4096):
                        out.append(_c(f"kmix{g}-{vname}-res-all-{k}-{n}", "b", ts, Ms, k, n, "plain", res=(0, 1, 2)))
                        out.append(_c(f"kmix{g}-{vname}-res-one-{k}-{n}", "b", ts, Ms, k, n, "plain", res=(1,)))
    types, Ms = Q80_GROUP
    for k in (1024, 4096):
        for n in (1, 4, 5):
            out.append(_c(f"q80-res-{k}-{n}", "b", types, Ms, k, n, "plain", res=(0, 1, 2)))
        for n in (1, 4):
            # the plan declines the mixed-format launch: per-type runs, each forming the norm itself
            out.append(_c(f"q80-norm-{k}-{n}", "b", types, Ms, k, n, "one_pass+two_step+two_step", norm=True))
    return out


GEOMETRY_ROWS = (2304, 1280, 40)             # 9, 5 and 1 rows per CU: 16-, 8- and 4-wave workgroups
# (name, K, N, norm, swiglu, residual)
GEOMETRY_FOLDS = (("norm", 4096, 1, True, 0, False), ("norm", 4096, 6, True, 0, False), ("norm", 5120, 5, True, 0, False),
                  ("swiglu-norm", 4096, 6, True, 1, False), ("res", 4096, 4, False, 0, True))


def cases_c(t):
    """geometry: the same weight rows in launches of 16, 8 and 4 waves; t = a family's type, or MIXED.  The mixed group puts its rows into the
    first matrix: (M - 32, 24, 8)"""
    out = []
    for fold, k, n, norm, swiglu, res in GEOMETRY_FOLDS:
        if t == MIXED and swiglu:
            continue
        for m in GEOMETRY_ROWS:
            if t == MIXED:
                types, Ms = KMIX_GROUPS[0][0], (m - 32, 24, 8)
            else:
                types, Ms = ((t, t), (m, m)) if swiglu else ((t,), (m,))
            path = (PATHS[k] if t == MIXED else norm_path(t, k)) if norm else "plain"
            out.append(_c(f"geo-{fold}-{k}-{n}-{m}", "c", types, Ms, k, n, path, norm=norm, swiglu=swiglu, res=tuple(range(len(Ms))) if res else ()))
    return out


def cases_d(t):
    """one-pass == two-step: the same norm launch in the default context and under GGML_MI355X_MV_ONEPASS=0; t = a Q8_K type, or MIXED"""
    out = []
    types = KMIX_GROUPS[0][0] if t == MIXED else (t,) * 3
    for k in ((2048, 4096) if t == Q6_KP else (1024, 4096)):
        for n in (1, 2, 6):
            out.append(_c(f"onepass-{k}-{n}", "d", types, GROUP_MS, k, n, "one_pass", norm=True))
            out.append(_c(f"onepass-off-{k}-{n}", "d", types, GROUP_MS, k, n, "two_step", norm=True, ctx="onepass=0"))
    return out


def cases_e(t):
    """sub-batches with a residual: 8 rows, tokens in two launches"""
    return [_c(f"subbatch-{k}-{n}", "e", (t,), (8,), k, n, "plain", res=(0,)) for k, n in ((16384, 8), (28672, 7))]


def cases_f(t):
    """activation value edges through the folds: K = 1024, 4 tokens (the rows and norm weights are the GPU test's)"""
    return [_c("edge-norm", "f", (t,) * 3, GROUP_MS, 1024, 4, norm_path(t, 1024), norm=True),
            _c("edge-norm-res", "f", (t,), (40,), 1024, 4, norm_path(t, 1024), norm=True, res=(0,)),
            _c("edge-swiglu-norm", "f", (t,) * 2, (24, 24), 1024, 4, norm_path(t, 1024), norm=True, swiglu=1)]


def cases_g():
    """refusals"""
    t = Q4_K
    return [_c("refuse-norm-7x4096", "g", (t,) * 3, GROUP_MS, 4096, 7, "refused", norm=True),
            _c("refuse-norm-6x5120", "g", (t,) * 3, GROUP_MS, 5120, 6, "refused", norm=True),
            _c("refuse-swiglu-rows", "g", (t,) * 2, (24, 40), 1024, 1, "refused", swiglu=1),
            _c("refuse-swiglu-res", "g", (t,) * 2, (24, 24), 1024, 1, "refused", swiglu=1, res=(0,))]


def q8k_types():
    return tuple(t for t in TYPES if act(t) == Q8_K)


def all_cases():
    """(key, case) of the whole table: key = the type (or MIXED, or None) the GPU tests parametrize the case by"""
    out = []
    for t in TYPES:
        out += [(t, c) for c in cases_a(t)]
    out += [(None, c) for c in cases_b()]
    for t in tuple(REPS.values()) + (MIXED,):
        out += [(t, c) for c in cases_c(t)]
    for t in q8k_types() + (MIXED,):
        out += [(t, c) for c in cases_d(t)]
    for t in REPS.values():
        out += [(t, c) for c in cases_e(t)] + [(t, c) for c in cases_f(t)]
    out += [(None, c) for c in cases_g()]
    return out


# ------------------------------------------------------------------------------------------------- the probe's notation

def probe_spec(case):
    """the case as a "group" spec of the plan probe of test_host_logic.py"""
    ex = ("n" if case.norm else "") + (f"s{case.swiglu}" if case.swiglu else "") + "".join(f"r{i}" for i in case.res)
    sw = CONTEXTS[case.ctx][1]
    return f"group {CUS} {','.join(map(str, case.types))} {','.join(map(str, case.Ms))} {case.K} {case.N} {ex or '-'}" + (f" {sw}" if sw else "")


def probe_line(case):
    """what the probe prints for the case's launches, or the refusal's text"""
    if case.refusal:
        return case.refusal
    return "; ".join(f"{label(l)} m={','.join(f'{i}:{r}' for i, r in zip(l.idx, l.rows))} n0={l.n0} grid={l.grid} block={l.waves * 64} lds={l.lds} arg={l.arg}"
                     for l in case.launches)


def labels_of(case):
    return tuple(label(l) for l in case.launches)
