"""GPU parity of GGML_OP_FLASH_ATTN_EXT's two kernels through the attention ABI (qmm_attn_decode / qmm_attn_prefill with
QMM_TENSOR_KV_ROWS on v, include/ggml_mi355x_ops.h): V arrives with cache positions as rows, the mask is f16 or f32, the result is the
merged-heads row the transposed-V launches write.  Checked against float64 numpy on the operands the kernels see (q and the mask rounded
to f16; ggml_compute_forward_flash_attn_ext_f16, ggml-cpu.c:10258-10471: scores in f32, s * scale + mask, p not rounded), in llama.cpp's
operand layout (strided cache views, a permuted q) and in the contiguous one of test-backend-ops.

Bars (max |err| / rms of the expected head block, as tests/test_gpu_layer_ops.py:297 holds this chain to): 5e-4 where a kernel rounds the
normalised p to f16, 1.5e-3 where it uses an unnormalised or f32 p.  Neither kernel here rounds p (f32 in the few-token kernel, an f16
pair in the prompt kernel), so every case stands at 1.5e-3; every measured value is printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F16 = 0, 1
BAR = 1.5e-3


@pytest.fixture(scope="module")
def qmm():
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    yield q
    q.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


def prefix_mask(n_tok, n_kv, rows=None):
    """every token sees a long prefix of the cache, each another one; one column is masked for all"""
    m = np.zeros((rows or (n_tok + 63) // 64 * 64, n_kv), np.float32)
    step = max(1, min(3, n_kv // 2 // max(n_tok - 1, 1)))
    for t in range(n_tok):
        m[t, n_kv - (n_tok - 1 - t) * step:] = -np.inf
    m[:, 5] = -np.inf
    return m


class Case:
    """operands on the host (q [h, n_tok, d], k / v [hk, n_kv, d], mask [rows, n_kv] of f16-representable values) and their expected result"""

    def __init__(self, n_tok, n_kv, d, h=8, hk=2, mask=None, seed=0):
        rng = np.random.default_rng(1000 * n_tok + n_kv + d + seed)
        self.n_tok, self.n_kv, self.d, self.h, self.hk = n_tok, n_kv, d, h, hk
        self.q = rng.normal(0, 1, (h, n_tok, d)).astype(np.float32)
        self.k = rng.normal(0, 1, (hk, n_kv, d)).astype(np.float16)
        self.v = rng.normal(0, 1, (hk, n_kv, d)).astype(np.float16)
        self.mask = (prefix_mask(n_tok, n_kv) if mask is None else mask).astype(np.float16).astype(np.float32)
        self.scale = 1.0 / np.sqrt(d)
        self._want = None

    def want(self):
        """[n_tok, h, d] in float64, computed once"""
        if self._want is None:
            qh = self.q.astype(np.float16).astype(np.float64)
            out = np.empty((self.n_tok, self.h, self.d))
            for hh in range(self.h):
                g = hh // (self.h // self.hk)
                s = qh[hh] @ self.k[g].astype(np.float64).T * np.float32(self.scale) + self.mask[:self.n_tok].astype(np.float64)
                p = np.exp(s - s.max(axis=1, keepdims=True))
                out[:, hh] = (p / p.sum(axis=1, keepdims=True)) @ self.v[g].astype(np.float64)
            self._want = out
        return self._want

    def run(self, qmm, layout="llama", mask_type=F16, entry=None, pitch=0):
        """one launch through the ABI; returns (result [n_tok, h, d], trace labels, the destination buffer with its guard columns)"""
        from ggml_hexagon_amd import capi
        n_tok, n_kv, d, h, hk = self.n_tok, self.n_kv, self.d, self.h, self.hk
        if layout == "llama":               # K / V: views of an [n_ctx, hk * d] cache; q: the permuted view of q_cur [d, h, n_tok]
            n_ctx = n_kv + 64
            kc, vc = (np.zeros((n_ctx, hk, d), np.float16) for _ in range(2))
            kc[:n_kv], vc[:n_kv] = self.k.transpose(1, 0, 2), self.v.transpose(1, 0, 2)
            kc[n_kv:], vc[n_kv:] = np.float16(np.nan), np.float16(np.nan)          # cache rows beyond n_kv are nobody's operand
            dq, dk, dvv = dev(self.q.transpose(1, 0, 2)), dev(kc), dev(vc)
            nbs = dict(q_nb=[4, h * d * 4, d * 4], k_nb=[2, hk * d * 2, d * 2], v_nb=[2, hk * d * 2, d * 2])
        else:                               # contiguous [d, n_kv, hk] and [d, n_tok, h], as test-backend-ops makes them
            dq, dk, dvv = dev(self.q), dev(self.k), dev(self.v)
            nbs = {}
        dm = dev(self.mask.astype(np.float16) if mask_type == F16 else self.mask)
        out = torch.full((n_tok, h * d + pitch), 7.0, device="cuda")
        ts = capi.flash_attn_operands(d, n_tok, h, hk, n_kv, q=dq.data_ptr(), k=dk.data_ptr(), v=dvv.data_ptr(), mask=dm.data_ptr(), dst=out.data_ptr(),
                                      mask_type=mask_type, mask_rows=self.mask.shape[0], dst_nb1=(h * d + pitch) * 4, **nbs)
        few = n_tok <= 8 if entry is None else entry == "decode"
        fn, sup = (qmm.lib.qmm_attn_decode, qmm.lib.qmm_attn_decode_supported) if few else (qmm.lib.qmm_attn_prefill, qmm.lib.qmm_attn_prefill_supported)
        r = [capi.C.byref(t) for t in ts]
        assert sup(*r) == 1
        labels = qmm.trace(lambda: qmm._chk(fn(qmm.ctx, *r, self.scale, qmm._stream())))
        qmm.synchronize()
        return out.cpu().numpy()[:, :h * d].reshape(n_tok, h, d), labels, out

    def check(self, got, what):
        want = self.want()
        errs = [rel_rms(got[:, hh], want[:, hh]) for hh in range(self.h)]
        print(f"{what} N={self.n_tok} n_kv={self.n_kv} D={self.d} H={self.h}/{self.hk}: max|err|/rms per head {max(errs):.3e} (bar {BAR:.1e})")
        assert np.isfinite(got).all()
        assert max(errs) <= BAR, (what, errs)


def decode_labels(d, n_kv):
    return (f"attn_rows_decode_kernel<{d}>",) + (("attn_combine_kernel",) if n_kv >= 1024 else ())


def prefill_labels(d):
    return (f"attn_rows_prefill_kernel<{d}>",)


# few tokens: one piece (D = 64 and 128), one below and one at the cut (960, 1024), ragged pieces (1088: 4 of 272), H_kv = H
DECODE_CASES = [(1, 256, 64, 8, 2), (3, 256, 128, 8, 2), (8, 512, 128, 8, 2), (2, 960, 128, 8, 2), (2, 1024, 128, 8, 2), (1, 1088, 64, 8, 2),
                (2, 2048, 128, 8, 8)]


@pytest.mark.parametrize("n_tok,n_kv,d,h,hk", DECODE_CASES, ids=["-".join(map(str, c)) for c in DECODE_CASES])
def test_flash_attn_few_tokens(qmm, n_tok, n_kv, d, h, hk):
    c = Case(n_tok, n_kv, d, h, hk)
    got, labels, _ = c.run(qmm)
    assert labels == decode_labels(d, n_kv), labels
    c.check(got, "few tokens")


# prompt batches: a ragged token tile, two token tiles, the least cache (LDS under 64 KiB: no limit raised), one chunk, the next multiple of
# 64 cache rows above a chunk (576), several chunks with a ragged last one (2304 = 4 x 512 + 256)
PREFILL_CASES = [(9, 256, 128), (33, 256, 64), (20, 64, 64), (70, 512, 128), (64, 576, 128), (130, 2304, 128)]


@pytest.mark.parametrize("n_tok,n_kv,d", PREFILL_CASES, ids=["-".join(map(str, c)) for c in PREFILL_CASES])
def test_flash_attn_prompt(qmm, n_tok, n_kv, d):
    c = Case(n_tok, n_kv, d)
    got, labels, _ = c.run(qmm)
    assert labels == prefill_labels(d), labels
    c.check(got, "prompt")


def test_flash_attn_first_generated_token_sees_forty_positions(qmm):
    """llama.cpp's first token after a 40-token prompt: the cache is padded to 256 rows, positions 40 .. 255 are masked; few tokens and,
    the same mask rows for a 40-token prompt, the prompt kernel (three of its four kv tiles are dead)"""
    for n_tok in (1, 40):
        m = np.full((64, 256), -np.inf, np.float32)
        for t in range(n_tok):
            m[t, :40 if n_tok == 1 else t + 1] = 0.0
        c = Case(n_tok, 256, 128, mask=m, seed=7)
        got, labels, _ = c.run(qmm)
        assert labels == (decode_labels(128, 256) if n_tok == 1 else prefill_labels(128)), labels
        c.check(got, "40 visible")


def test_flash_attn_padded_mask_rows_are_all_masked(qmm):
    """the mask has 64 rows for 33 tokens and the padding rows are -inf throughout, as llama.cpp fills them: they belong to no token, a
    token tile's clamped rows repeat token 32's"""
    m = prefix_mask(33, 256)
    m[33:] = -np.inf
    c = Case(33, 256, 128, mask=m, seed=3)
    got, labels, _ = c.run(qmm)
    assert labels == prefill_labels(128), labels
    c.check(got, "padded rows masked")


def test_flash_attn_causal_mask_kills_whole_kv_tiles(qmm):
    """a causal prompt at the end of a cache of 704 rows (two chunks): token t sees positions 0 .. 574 + t, so for the first 64 tokens the
    last kv tile (640 .. 703) is dead; the second token tile has every tile alive"""
    n_tok, n_kv = 130, 704
    m = np.full((192, n_kv), -np.inf, np.float32)
    for t in range(n_tok):
        m[t, :n_kv - n_tok + t + 1] = 0.0
    c = Case(n_tok, n_kv, 128, mask=m, seed=5)
    got, labels, _ = c.run(qmm)
    assert labels == prefill_labels(128), labels
    c.check(got, "causal, dead tiles")
    # ... and a prompt on an empty cache: whole chunks are dead for the first token tile
    n_tok = n_kv = 576
    m = np.full((n_tok, n_kv), -np.inf, np.float32)
    for t in range(n_tok):
        m[t, :t + 1] = 0.0
    c = Case(n_tok, n_kv, 64, h=4, hk=2, mask=m, seed=6)
    got, labels, _ = c.run(qmm)
    c.check(got, "causal from an empty cache")


@pytest.mark.parametrize("n_tok,n_kv,d", [(3, 512, 128), (35, 512, 64), (2, 1024, 64)], ids=["3-512-128", "35-512-64", "2-1024-64"])
def test_flash_attn_contiguous_operands_and_finite_masks(qmm, n_tok, n_kv, d):
    """test-backend-ops' operands: contiguous K / V / q, H_kv = H / 4 and a mask of random finite values; an f32 and an f16 mask of the same
    values give the same bits"""
    rng = np.random.default_rng(n_tok)
    m = rng.uniform(-1, 1, (64, n_kv)).astype(np.float32)
    c = Case(n_tok, n_kv, d, h=16, hk=4, mask=m, seed=11)
    got16, labels, _ = c.run(qmm, layout="contiguous", mask_type=F16)
    assert labels == (decode_labels(d, n_kv) if n_tok <= 8 else prefill_labels(d)), labels
    c.check(got16, "contiguous, finite f16 mask")
    got32, _, _ = c.run(qmm, layout="contiguous", mask_type=F32)
    c.check(got32, "contiguous, finite f32 mask")
    assert np.array_equal(got16.view(np.int32), got32.view(np.int32))
    got_l, _, _ = c.run(qmm, layout="llama", mask_type=F16)
    assert np.array_equal(got16.view(np.int32), got_l.view(np.int32))            # the layout moves addresses, not arithmetic


@pytest.mark.parametrize("n_tok,n_kv", [(2, 256), (2, 1024), (70, 256)], ids=["2-256", "2-1024", "70-256"])
def test_flash_attn_destination_pitch_and_guard_columns(qmm, n_tok, n_kv):
    c = Case(n_tok, n_kv, 128, seed=13)
    got, _, out = c.run(qmm, pitch=16)
    c.check(got, "pitched destination")
    assert torch.equal(out[:, 8 * 128:], torch.full((n_tok, 16), 7.0, device="cuda"))


@pytest.mark.parametrize("n_tok,n_kv,d", [(2, 512, 128), (9, 256, 128)], ids=["2-512-128", "9-256-128"])
def test_flash_attn_agrees_with_the_transposed_launches(qmm, n_tok, n_kv, d):
    """the same data with V transposed on the host through the existing flags = 0 entry points (which round the normalised p to f16)"""
    from ggml_hexagon_amd import capi
    c = Case(n_tok, n_kv, d, seed=17)
    got, _, _ = c.run(qmm)
    h, hk = c.h, c.hk
    dq, dk, dvt, dm = dev(c.q), dev(c.k), dev(c.v.transpose(0, 2, 1)), dev(c.mask)
    out = torch.empty((n_tok, h * d), device="cuda")
    T = capi.QmmTensor.make
    ts = (T(F32, [d, n_tok, h], data=dq.data_ptr()), T(F16, [d, n_kv, hk], data=dk.data_ptr()), T(F16, [n_kv, d, hk], data=dvt.data_ptr()),
          T(F32, [n_kv, c.mask.shape[0]], data=dm.data_ptr()), T(F32, [h * d, n_tok], data=out.data_ptr()))
    fn = qmm.lib.qmm_attn_decode if n_tok <= 8 else qmm.lib.qmm_attn_prefill
    labels = qmm.trace(lambda: qmm._chk(fn(qmm.ctx, *[capi.C.byref(t) for t in ts], c.scale, qmm._stream())))
    assert not any("rows" in l for l in labels), labels
    other = out.cpu().numpy().reshape(n_tok, h, d)
    errs = [rel_rms(got[:, hh], other[:, hh]) for hh in range(h)]
    print(f"against the transposed launch N={n_tok} n_kv={n_kv}: max|diff|/rms per head {max(errs):.3e} (bar {BAR:.1e})")
    assert max(errs) <= BAR, errs
    c.check(got, "cross-check")


@pytest.mark.parametrize("n_tok,n_kv", [(3, 256), (3, 2048), (130, 1088)], ids=["3-256", "3-2048", "130-1088"])
def test_flash_attn_is_deterministic(qmm, n_tok, n_kv):
    c = Case(n_tok, n_kv, 128, seed=19)
    a, _, _ = c.run(qmm)
    b, _, _ = c.run(qmm)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_flash_attn_entry_points_overlap_at_few_tokens(qmm):
    """qmm_attn_prefill takes any N: three tokens through the prompt kernel (the plugin's route for a cache past the few-token limit)"""
    c = Case(3, 256, 64, seed=23)
    got, labels, _ = c.run(qmm, entry="prefill")
    assert labels == prefill_labels(64), labels
    c.check(got, "3 tokens, prompt kernel")
