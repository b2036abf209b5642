"""Times of the launches a K cache in Q4_0, Q4_1, Q5_0 or Q5_1 adds (csrc/qmm_kblk.hiph) beside the F16-cache and the Q8_0-cache launches of
the same library on the same shapes and values, all through the C-ABI of include/ggml_mi355x_ops.h.

    python profiles/tools/kblk_times.py [--out profiles/kblk_attn_times.txt]

Per shape: 20 warm-up calls per variant, then 15 windows of 200 back-to-back calls between two device events, the six variants alternating
window by window; the figure is the median window / 200 (us per call, launch gaps included; operands of these sizes stay in the caches).
llama3-8b's heads: H = 32, H_kv = 8, D = 128, llama.cpp's operand layout (strided cache views, permuted q), causal masks.
  few tokens / prompt   qmm_attn_decode / qmm_attn_prefill on an F16 K cache and on the same K rows in Q8_0 and in each of the four types
  store, one token      F16 cache: qmm_rope_kv_store(q, k, v), one launch; a quantized K cache: qmm_rope_kv_store(q, v) + ROPE(k) + CPY f32 -> type"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import kblk_refs as R  # noqa: E402
from ggml_hexagon_amd import capi  # noqa: E402

F32, F16, Q8_0, I32 = 0, 1, 8, 26
H, HK, D = 32, 8, 128
BLOCK = dict(R.BLOCK)
BLOCK[Q8_0] = 34
NAMES = dict(R.NAMES)
NAMES[Q8_0] = "q8_0"
KTYPES = (Q8_0,) + R.TYPES
SHAPES = [("few tokens", 1, 512), ("few tokens", 1, 4096), ("few tokens", 1, 16384), ("prompt", 512, 512), ("prompt", 512, 4096)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def q8_rows(x):
    """block_q8_0 bytes of f32 rows (d = amax / 127 as f16, q = rint(x / d)): values for timing, not a reference"""
    b = x.reshape(x.shape[0], -1, 32)
    d = (np.abs(b).max(axis=2, keepdims=True) / 127.0).astype(np.float16)
    q = np.rint(b / np.maximum(d.astype(np.float32), 1e-30)).clip(-127, 127).astype(np.int8)
    out = np.zeros(b.shape[:2] + (34,), np.uint8)
    out[:, :, 0:2] = d.view(np.uint8).reshape(b.shape[0], -1, 2)
    out[:, :, 2:] = q.view(np.uint8)
    return out.reshape(x.shape[0], -1)


def timed(runs, windows, launches):
    for call, _ in runs:
        for _ in range(20):
            call()
    torch.cuda.synchronize()
    for _ in range(windows):
        for call, times in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1000.0 / launches)
    return [statistics.median(t) for _, t in runs]


def f2i(x):
    return int(np.float32(x).view(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kblk_attn_times.txt"))
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = capi.Qmm(0)
    T, r = capi.QmmTensor.make, capi.C.byref
    lines = [f"# us per call, median of {a.windows} windows of {a.launches} calls (profiles/tools/kblk_times.py); H={H} H_kv={HK} D={D}",
             "# family      N   n_kv  K cache  launch(es)                                                         us  / F16  / Q8_0  max|diff|/rms to F16"]
    scale = 1.0 / np.sqrt(D)
    for family, n_tok, n_kv in SHAPES:
        rng = np.random.default_rng(n_tok + n_kv)
        n_ctx = n_kv + 256
        q = dev(rng.normal(0, 1, (n_tok, H, D)).astype(np.float32))
        kf = rng.normal(0, 1, (n_ctx * HK, D)).astype(np.float32)
        vt = dev(rng.normal(0, 1, (HK, D, n_ctx)).astype(np.float16))
        rows = (n_tok + 63) // 64 * 64
        m = np.full((rows, n_kv), -np.inf, np.float32)
        for t in range(n_tok):
            m[t, :n_kv - n_tok + t + 1] = 0.0
        m = dev(m)
        tq = T(F32, [D, n_tok, H], nb=[4, H * D * 4, D * 4, n_tok * H * D * 4], data=q.data_ptr())
        tv = T(F16, [n_kv, D, HK], nb=[2, n_ctx * 2, n_ctx * D * 2, n_ctx * D * HK * 2], data=vt.data_ptr())
        tm = T(F32, [n_kv, rows], data=m.data_ptr())
        few = n_tok <= 8
        fn = lib.lib.qmm_attn_decode if few else lib.lib.qmm_attn_prefill
        keep = [dev(kf.astype(np.float16))]
        tks = [("f16", T(F16, [D, n_kv, HK], nb=[2, HK * D * 2, D * 2, n_ctx * HK * D * 2], data=keep[0].data_ptr()))]
        for kt in KTYPES:
            keep.append(dev(q8_rows(kf) if kt == Q8_0 else R.quantize(kt, kf)))
            hb = D // 32 * BLOCK[kt]
            tks.append((NAMES[kt], T(kt, [D, n_kv, HK], nb=[BLOCK[kt], HK * hb, hb, n_ctx * HK * hb], data=keep[-1].data_ptr())))
        runs, labels, outs = [], [], []
        for _, tk in tks:
            outs.append(torch.zeros((n_tok, H * D), device="cuda"))
            refs = [r(tq), r(tk), r(tv), r(tm), r(T(F32, [H * D, n_tok], data=outs[-1].data_ptr()))]
            call = (lambda refs=refs: lib._chk(fn(lib.ctx, *refs, scale, lib._stream())))
            labels.append(lib.trace(call))
            runs.append((call, []))
        us = timed(runs, a.windows, a.launches)
        o = outs[0].cpu().numpy().astype(np.float64)
        for i, (name, _) in enumerate(tks):
            n = outs[i].cpu().numpy().astype(np.float64)
            diff = float(np.max(np.abs(o - n)) / np.sqrt(np.mean(o ** 2)))          # (the quantized rows are another K: quantization, not kernel error)
            lines.append(f"{family:<11} {n_tok:>4} {n_kv:>6}  {name:<7}  {'+'.join(labels[i]):<62} {us[i]:>7.1f}  {us[i] / us[0]:>5.2f}  {us[i] / us[1]:>6.2f}  {diff:.1e}")
            print(lines[-1], flush=True)
    # the store of one token
    n_ctx, j0 = 4096, 1000
    rope = [0, D, 0, 0, 8192, f2i(500000.0), f2i(1.0), f2i(0.0), f2i(1.0), f2i(32.0), f2i(1.0)]
    rng = np.random.default_rng(7)
    qc, kc, vc = (dev(rng.normal(0, 1, (1, h, D)).astype(np.float32)) for h in (H, HK, HK))
    pos = dev(np.array([j0], np.int32))
    qd, kr = torch.zeros_like(qc), torch.zeros_like(kc)
    kcache16 = torch.zeros((n_ctx, HK * D), dtype=torch.float16, device="cuda")
    kcacheq = torch.zeros((n_ctx, HK * D // 32 * 34), dtype=torch.uint8, device="cuda")
    vcache = torch.zeros((HK * D, n_ctx), dtype=torch.float16, device="cuda")
    tq, tqd = T(F32, [D, H, 1], data=qc.data_ptr()), T(F32, [D, H, 1], data=qd.data_ptr(), op_params=rope)
    tk, tkr = T(F32, [D, HK, 1], data=kc.data_ptr()), T(F32, [D, HK, 1], data=kr.data_ptr(), op_params=rope)
    tpos = T(I32, [1], data=pos.data_ptr())
    tkd16 = T(F16, [D, HK, 1], data=kcache16.data_ptr() + j0 * HK * D * 2)
    tv = T(F32, [1, HK * D], nb=[HK * D * 4, 4, HK * D * 4, HK * D * 4], data=vc.data_ptr())
    tvd = T(F16, [1, HK * D], nb=[2, n_ctx * 2, n_ctx * HK * D * 2, n_ctx * HK * D * 2], data=vcache.data_ptr() + j0 * 2)
    store = lib.lib.qmm_rope_kv_store

    def f16_store():
        lib._chk(store(lib.ctx, r(tq), r(tpos), None, r(tqd), r(tk), r(tkd16), r(tv), r(tvd), lib._stream()))

    def quant_store(tkd):
        def run():
            lib._chk(store(lib.ctx, r(tq), r(tpos), None, r(tqd), None, None, r(tv), r(tvd), lib._stream()))
            lib.op(capi.OP_ROPE, tkr, tk, tpos)
            lib.op(capi.OP_CPY, tkd, tkr)
        return run

    runs, names = [(f16_store, [])], ["qmm_rope_kv_store(q, k, v): 1 launch"]
    for kt in KTYPES:
        row = HK * D // 32 * BLOCK[kt]
        call = quant_store(T(kt, [HK * D], nb=[BLOCK[kt], row, row, row], data=kcacheq.data_ptr() + j0 * row))
        names.append("qmm_rope_kv_store(q, v)+" + "+".join(lib.trace(call)))              # (the traced launches: ROPE(k) and the CPY)
        runs.append((call, []))
    us = timed(runs, a.windows, a.launches)
    lines.append("# the store of one token (rope(q), rope(k) -> K cache, v -> V cache):")
    for i, name in enumerate(names):
        lines.append(f"store          1 {'':>6}  {'f16' if i == 0 else NAMES[KTYPES[i - 1]]:<7}  {name:<62} {us[i]:>7.1f}  {us[i] / us[0]:>5.2f}  {us[i] / us[1]:>6.2f}")
        print(lines[-1], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
