"""qmm_rope_kq_store on the GPU: rope(q), rope(k) into a K cache of Q8_0, Q4_0, Q4_1, Q5_0 or Q5_1 blocks and the V store as one launch
(csrc/qmm_ropekq.hiph).  The oracle is the library's own three-launch path on the same inputs in the same context:
qmm_rope_kv_store(q, .., NULL, NULL, v, v_dst), ROPE of k into a contiguous f32 tensor, CPY of that into cache A; the new entry point writes
cache B, q_dst B and V cache B, and every byte must agree.  One independent line per type checks the dequantized rows against the numpy rope."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import glue_refs  # noqa: E402
import kblk_refs  # noqa: E402
from oracle.pyoracle import ACT_REF, ACT_X86  # noqa: E402

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, I32 = 0, 1, 2, 3, 6, 7, 8, 26
BLOCK = {Q8_0: 34, Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24}
NAMES = {Q8_0: "q8_0", Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1"}
# Q8_0 blocks depend on the context's act mode (the reference quantizer or the x86 one); the other four do not
TYPE_MODES = [(Q8_0, ACT_REF), (Q8_0, ACT_X86), (Q4_0, ACT_REF), (Q4_1, ACT_REF), (Q5_0, ACT_REF), (Q5_1, ACT_REF)]
TYPE_MODE_IDS = ["q8_0-ref", "q8_0-x86", "q4_0", "q4_1", "q5_0", "q5_1"]

J0, GUARD = 3, 2                    # the batch's first cache row; zeroed rows kept behind the batch


@pytest.fixture(scope="module")
def qmm():
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    yield q
    q.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f2i(x):
    return int(np.float32(x).view(np.int32))


# (tokens, variant): the words of a variant, in any order
#   neox / partial (n_dims 64 of D = 128) / ff (frequency factors) / yarn (ext_factor 1, freq_scale 0.25: the ramp)
#   d64 (D = 64, one q head, one kv head: with no v the smallest launch, 2 blocks) / d256 / hk3 (12 and 3 heads: a short head chunk) / hk8 (32 and 8)
#   nov (no v pair) / vrows (v and v_dst both dense rows: element-wise at any N; otherwise v_cur^T into the transposed cache, tiles from 32 tokens on)
#   kview (k's tokens further apart than H_kv * D * 4 bytes) / edges (value edges in pass-through channels and whole heads, see edge_heads)
CASES = [(1, "normal"), (5, "normal"), (70, "normal"), (5, "neox"), (70, "neox"), (5, "partial"), (5, "neox-partial"), (5, "ff"), (70, "neox-ff"), (5, "yarn"),
         (70, "neox-yarn-ff"), (1, "d64-nov"), (5, "d64"), (5, "hk3"), (70, "hk3-neox-partial-ff"), (1, "hk8"), (5, "hk8"), (5, "d256"), (70, "d256-neox"),
         (5, "nov"), (70, "nov"), (70, "vrows"), (5, "vrows"), (5, "kview"), (70, "kview-neox"), (1, "edges"), (5, "edges"), (70, "edges-neox")]
CASE_IDS = [f"{n}-{v}" for n, v in CASES]


def edge_heads(k, n_dims):
    """value edges for K that pass through the rope, in token 0 of a [n, 4, 128] batch with n_dims = 64 (channels 64 .. 127 are copied):
    head 0 all zero (the d = -0 block of the Q4_0 / Q5_0 quantizers); head 1: a block whose largest magnitude is negative, and a block of one
    repeated value (the _1 types' d = 0); head 2: a block holding 65504 and 1e-8, and a block of 1e-8 alone"""
    assert k.shape[1] == 4 and k.shape[2] == 128 and n_dims == 64
    k[0, 0, :] = 0.0
    k[0, 1, 64:96] = -np.abs(k[0, 1, 64:96])
    k[0, 1, 70] = -7.5
    k[0, 1, 96:128] = 0.3
    k[0, 2, 64:96:2] = 65504.0
    k[0, 2, 65:96:2] = 1e-8
    k[0, 2, 96:128] = 1e-8


def build_case(n, variant, seed):
    w = set(variant.split("-"))
    d = 64 if "d64" in w else 256 if "d256" in w else 128
    h, hk = (1, 1) if "d64" in w else (12, 3) if "hk3" in w else (32, 8) if "hk8" in w else (8, 4) if "edges" in w else (8, 2)
    n_dims = 64 if ("partial" in w or "edges" in w) else d
    rng = np.random.default_rng(seed)
    c = {"n": n, "d": d, "h": h, "hk": hk, "n_dims": n_dims, "neox": "neox" in w, "words": w}
    c["ff"] = rng.uniform(0.8, 4.0, n_dims // 2).astype(np.float32) if "ff" in w else None
    c["q"] = rng.normal(0, 1, (n, h, d)).astype(np.float32)
    c["k"] = rng.normal(0, 1, (n, hk, d)).astype(np.float32)
    c["v"] = None if "nov" in w else rng.normal(0, 1, (n, hk * d)).astype(np.float32)
    c["pos"] = np.arange(17, 17 + n, dtype=np.int32)
    if "edges" in w:
        edge_heads(c["k"], n_dims)
    yarn = "yarn" in w
    c["rope_kw"] = dict(freq_scale=0.25, ext_factor=1.0) if yarn else {}
    c["params"] = [0, n_dims, 2 if c["neox"] else 0, 0, 8192, f2i(10000.0), f2i(0.25 if yarn else 1.0), f2i(1.0 if yarn else 0.0), f2i(1.0), f2i(32.0), f2i(1.0)]
    return c


def run_both(qmm, t, c):
    """the three existing launches into (q_dst, K cache, V cache) A and the new launch into B; returns both triples as numpy and B's trace"""
    from ggml_hexagon_amd import capi
    T = capi.QmmTensor.make
    n, d, h, hk, w = c["n"], c["d"], c["h"], c["hk"], c["words"]
    n_ctx = J0 + n + GUARD
    row = hk * d // 32 * BLOCK[t]
    dq, dpos = dev(c["q"]), dev(c["pos"])
    dff = dev(c["ff"]) if c["ff"] is not None else None
    if "kview" in w:
        pad = np.zeros((n, hk * d + 64), np.float32)
        pad[:, :hk * d] = c["k"].reshape(n, -1)
        dk = dev(pad)
        k_nb = [4, d * 4, (hk * d + 64) * 4, (hk * d + 64) * 4 * n]
    else:
        dk, k_nb = dev(c["k"]), None
    tq, tpos = T(F32, [d, h, n], data=dq.data_ptr()), T(I32, [n], data=dpos.data_ptr())
    tff = T(F32, [c["n_dims"] // 2], data=dff.data_ptr()) if dff is not None else None
    tk = T(F32, [d, hk, n], nb=k_nb, data=dk.data_ptr())
    dv = dev(c["v"]) if c["v"] is not None else None
    r = lambda x: capi.C.byref(x) if x is not None else None
    out = []
    trace = None
    for new in (False, True):
        q_out = torch.zeros_like(dq)
        k_cache = torch.zeros((n_ctx, row), dtype=torch.uint8, device="cuda")
        tqo = T(F32, [d, h, n], data=q_out.data_ptr(), op_params=c["params"])
        tkd = T(t, [d, hk, n], nb=[BLOCK[t], d // 32 * BLOCK[t], row, row * n], data=k_cache.data_ptr() + J0 * row)
        tv = tvd = v_cache = None
        if dv is not None and "vrows" in w:
            v_cache = torch.zeros((n_ctx, hk * d), dtype=torch.float16, device="cuda")
            tv = T(F32, [hk * d, n], data=dv.data_ptr())
            tvd = T(F16, [hk * d, n], data=v_cache.data_ptr() + J0 * hk * d * 2)
        elif dv is not None:
            v_cache = torch.zeros((hk * d, n_ctx), dtype=torch.float16, device="cuda")
            tv = T(F32, [n, hk * d], nb=[hk * d * 4, 4, 4 * n * hk * d, 4 * n * hk * d], data=dv.data_ptr())                 # v_cur^T
            tvd = T(F16, [n, hk * d], nb=[2, n_ctx * 2, n_ctx * 2 * hk * d, n_ctx * 2 * hk * d], data=v_cache.data_ptr() + J0 * 2)
        if new:
            assert qmm.lib.qmm_rope_kq_store_supported(r(tq), r(tpos), r(tff), r(tqo), r(tk), r(tkd), r(tv), r(tvd)) == 1
            trace = qmm.trace(lambda: qmm._chk(qmm.lib.qmm_rope_kq_store(qmm.ctx, r(tq), r(tpos), r(tff), r(tqo), r(tk), r(tkd), r(tv), r(tvd), qmm._stream())))
        else:
            assert qmm.lib.qmm_rope_kv_store_supported(r(tq), r(tpos), r(tff), r(tqo), None, None, r(tv), r(tvd)) == 1
            qmm._chk(qmm.lib.qmm_rope_kv_store(qmm.ctx, r(tq), r(tpos), r(tff), r(tqo), None, None, r(tv), r(tvd), qmm._stream()))
            k_roped = torch.zeros((n, hk, d), dtype=torch.float32, device="cuda")
            tkr = T(F32, [d, hk, n], data=k_roped.data_ptr(), op_params=c["params"])
            qmm.op(capi.OP_ROPE, tkr, tk, tpos, tff)
            qmm.op(capi.OP_CPY, tkd, tkr)
        qmm.synchronize()
        out.append((q_out.cpu().numpy(), k_cache.cpu().numpy(), v_cache.cpu().numpy() if v_cache is not None else None))
    return out[0], out[1], trace


def v_form(c):
    """the v part the plan takes: tiles for v_cur^T of at least 32 tokens"""
    return "true" if c["v"] is not None and "vrows" not in c["words"] and c["n"] >= 32 else "false"


@pytest.mark.parametrize("n,variant", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("t,act_mode", TYPE_MODES, ids=TYPE_MODE_IDS)
def test_one_launch_writes_the_bytes_of_the_three(qmm, t, act_mode, n, variant):
    c = build_case(n, variant, seed=100 * n + len(variant))
    qmm.set_act_mode(act_mode)
    try:
        (qa, ka, va), (qb, kb, vb), trace = run_both(qmm, t, c)
    finally:
        qmm.set_act_mode(ACT_REF)
    assert trace == (f"rope_kq_store_kernel<{NAMES[t]},{v_form(c)}>",), trace
    assert ka[J0:J0 + n].any() and qa.any()                                           # the oracle path has written
    assert np.array_equal(kb[J0:J0 + n], ka[J0:J0 + n]), np.flatnonzero(kb != ka)[:8]
    assert not kb[:J0].any() and not kb[J0 + n:].any()                                # guard rows in front of and behind the batch
    assert np.array_equal(qb.view(np.int32), qa.view(np.int32))
    if va is None:
        assert vb is None
    else:
        assert va.any() and np.array_equal(vb.view(np.uint16), va.view(np.uint16))
        if "vrows" in c["words"]:
            assert not vb[:J0].any() and not vb[J0 + n:].any()
        else:                                                                         # the transposed cache: the bytes between dst rows
            assert not vb[:, :J0].any() and not vb[:, J0 + n:].any()
    if "edges" in c["words"]:                                                         # the edge blocks are what they were built to be
        blocks = kb[J0].reshape(c["hk"], c["d"] // 32, BLOCK[t])
        d0 = blocks[0, :, :2].copy().view(np.uint16)
        assert ((d0 & 0x7FFF) == 0).all() and (t not in (Q4_0, Q5_0) or (d0 == 0x8000).all())          # d = -0 where max / -8 is formed
        if t in (Q4_1, Q5_1):
            assert ((blocks[1, 3, :2].copy().view(np.uint16) & 0x7FFF) == 0).all()                  # one repeated value: d = 0


@pytest.mark.parametrize("t,act_mode", TYPE_MODES, ids=TYPE_MODE_IDS)
def test_rows_against_the_numpy_rope(qmm, oracle, t, act_mode):
    """Independent of the library's own launches: the rows of cache B, dequantized, against r = glue_refs.rope(k) (cos / sin in double).  The
    relation, per block, with e_b = max |deq(B) - r| and e_ref = max |deq(Q_ref(r)) - r| the reference quantizer's own error on the same
    roped block:  e_b <= e_ref + 2 (A + eps),  A = c_max 2^-10 |d_ref| [+ 2^-10 |m_ref|],  eps = 2^-21 max |k| over the head.
    eps is what the device's f32 rope can differ from r by: cos and sin to an ulp of 1 (2^-23 each), two rounded products and a rounded
    sum (2^-24 each) on a pair whose members are at most max |k|: under 4 * 2^-23 max |k|.  A is what that can move in the scales: an amax or
    min that differs rounds d (and m) to the neighbouring f16, one ulp (2^-10 relative), which moves a dequantized value by at most c_max
    (the type's largest code magnitude) ulps of d.  An element whose code is the reference's is therefore within A + eps of the
    reference's error.  An element whose code is the neighbour of the reference's lay within A + eps of a code boundary: there the
    reference's own error is at least |d| / 2 - (A + eps), so e_ref is, and the element's error is at most |d| / 2 + A + eps.  No step of d
    is granted anywhere, and no number is fitted to what the kernel gives."""
    n, variant = 5, "hk3"
    c = build_case(n, variant, seed=11)
    qmm.set_act_mode(act_mode)
    try:
        _, (_, kb, _), _ = run_both(qmm, t, c)
    finally:
        qmm.set_act_mode(ACT_REF)
    d, hk = c["d"], c["hk"]
    r = glue_refs.rope(c["k"][None], c["pos"], c["n_dims"], neox=c["neox"], ff=c["ff"], **c["rope_kw"])[0].astype(np.float32).reshape(n, hk * d)
    rows = kb[J0:J0 + n]
    if t == Q8_0:
        ref = oracle.quantize_act(Q8_0, r, act_mode)
        deq = lambda w: oracle.dequantize(Q8_0, w, hk * d)
        cmax = 127
    else:
        ref = kblk_refs.quantize(t, r)
        deq = lambda w: kblk_refs.dequantize(t, w, hk * d)
        cmax = {Q4_0: 8, Q4_1: 15, Q5_0: 16, Q5_1: 31}[t]
    rb = r.reshape(-1, 32).astype(np.float64)
    e_b = np.abs(deq(rows).reshape(-1, 32) - rb).max(axis=1)
    e_ref = np.abs(deq(ref).reshape(-1, 32) - rb).max(axis=1)
    refb = ref.reshape(-1, BLOCK[t])
    d_ref = np.abs(refb[:, 0:2].copy().view(np.float16).astype(np.float64)[:, 0])
    m_ref = np.abs(refb[:, 2:4].copy().view(np.float16).astype(np.float64)[:, 0]) if t in (Q4_1, Q5_1) else np.zeros_like(d_ref)
    eps = np.repeat(np.abs(c["k"]).max(axis=2).reshape(-1), d // 32).astype(np.float64) * 2.0 ** -21
    bound = e_ref + 2.0 * (cmax * 2.0 ** -10 * d_ref + 2.0 ** -10 * m_ref + eps)
    same = int((rows.reshape(-1, BLOCK[t]) == refb).all(axis=1).sum())
    print(f"{NAMES[t]}: max block error {e_b.max():.4g} (reference quantizer on the same rows {e_ref.max():.4g}); worst e_b / bound {np.max(e_b / bound):.3f}; "
          f"{same} of {len(refb)} blocks are the reference's bytes")
    assert (e_b <= bound).all()
