"""Times of the launches a Q8_0 K cache adds (csrc/qmm_kcache.hiph) beside the F16-cache launches of the same library on the same shapes and
values, all through the C-ABI of include/ggml_mi355x_ops.h.

    python profiles/tools/kq8_times.py [--out profiles/kq8_attn_times.txt]

Per shape and variant: 20 warm-up calls, then 15 windows of 200 back-to-back calls between two device events, the variants alternating
window by window; the figure is the median window / 200 (us per call, launch gaps included; operands of these sizes stay in the caches).
llama3-8b's heads: H = 32, H_kv = 8, D = 128, llama.cpp's operand layout (strided cache views, permuted q), causal masks.
  few tokens / prompt   qmm_attn_decode / qmm_attn_prefill on an F16 K cache and on the same K rows as Q8_0; for the prompt the unpack launch
                        (Q8_0 -> f16 image of the rows the batch reads) is also timed on its own, as the CPY it is
  store, one token      F16 cache: qmm_rope_kv_store(q, k, v), one launch; Q8_0 K cache: qmm_rope_kv_store(q, v) + ROPE(k) + CPY f32 -> Q8_0"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from ggml_hexagon_amd import capi  # noqa: E402

F32, F16, Q8_0, I32 = 0, 1, 8, 26
H, HK, D = 32, 8, 128
HB = D // 32 * 34
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kq8_attn_times.txt"))
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = capi.Qmm(0)
    T, r = capi.QmmTensor.make, capi.C.byref
    lines = [f"# us per call, median of {a.windows} windows of {a.launches} calls (profiles/tools/kq8_times.py); H={H} H_kv={HK} D={D}",
             "# family      N   n_kv  F16 K cache launch(es)                              us   Q8_0 K cache launch(es)                                      us  ratio  max|diff|/rms"]
    scale = 1.0 / np.sqrt(D)
    for family, n_tok, n_kv in SHAPES:
        rng = np.random.default_rng(n_tok + n_kv)
        n_ctx = n_kv + 256
        q = dev(rng.normal(0, 1, (n_tok, H, D)).astype(np.float32))
        kf = rng.normal(0, 1, (n_ctx * HK, D)).astype(np.float32)
        k16, k8 = dev(kf.astype(np.float16)), dev(q8_rows(kf))
        vt = dev(rng.normal(0, 1, (HK, D, n_ctx)).astype(np.float16))
        rows = (n_tok + 63) // 64 * 64
        m = np.full((rows, n_kv), -np.inf, np.float32)
        for t in range(n_tok):
            m[t, :n_kv - n_tok + t + 1] = 0.0
        m = dev(m)
        outs = [torch.zeros((n_tok, H * D), device="cuda") for _ in range(2)]
        tq = T(F32, [D, n_tok, H], nb=[4, H * D * 4, D * 4, n_tok * H * D * 4], data=q.data_ptr())
        tk16 = T(F16, [D, n_kv, HK], nb=[2, HK * D * 2, D * 2, n_ctx * HK * D * 2], data=k16.data_ptr())
        tk8 = T(Q8_0, [D, n_kv, HK], nb=[34, HK * HB, HB, n_ctx * HK * HB], data=k8.data_ptr())
        tv = T(F16, [n_kv, D, HK], nb=[2, n_ctx * 2, n_ctx * D * 2, n_ctx * D * HK * 2], data=vt.data_ptr())
        tm = T(F32, [n_kv, rows], data=m.data_ptr())
        few = n_tok <= 8
        fn = lib.lib.qmm_attn_decode if few else lib.lib.qmm_attn_prefill
        runs, labels = [], []
        for tk, out in ((tk16, outs[0]), (tk8, outs[1])):
            refs = [r(tq), r(tk), r(tv), r(tm), r(T(F32, [H * D, n_tok], data=out.data_ptr()))]
            call = (lambda refs=refs: lib._chk(fn(lib.ctx, *refs, scale, lib._stream())))
            labels.append(lib.trace(call))
            runs.append((call, []))
        if not few:                                      # the unpack launch on its own: the same rows into a contiguous f16 image
            img = torch.zeros((HK, n_kv, D), dtype=torch.float16, device="cuda")
            timg = T(F16, [D, n_kv, HK], data=img.data_ptr())
            call = lambda: lib.op(capi.OP_CPY, timg, tk8)
            labels.append(lib.trace(call))
            runs.append((call, []))
        us = timed(runs, a.windows, a.launches)
        o, n = outs[0].cpu().numpy().astype(np.float64), outs[1].cpu().numpy().astype(np.float64)
        diff = float(np.max(np.abs(o - n)) / np.sqrt(np.mean(o ** 2)))           # (the Q8_0 rows are another K: quantization, not kernel error)
        lines.append(f"{family:<11} {n_tok:>4} {n_kv:>6}  {'+'.join(labels[0]):<48} {us[0]:>7.1f}   {'+'.join(labels[1]):<56} {us[1]:>7.1f}  {us[1] / us[0]:>5.2f}  {diff:.1e}")
        print(lines[-1], flush=True)
        if not few:
            lines.append(f"{'':<11} {'':>4} {'':>6}  {'':<48} {'':>7}   {'the unpack launch alone: ' + '+'.join(labels[2]):<56} {us[2]:>7.1f}")
            print(lines[-1], flush=True)
    # the store of one token
    n_ctx, j0 = 4096, 1000
    rope = [0, D, 0, 0, 8192, f2i(500000.0), f2i(1.0), f2i(0.0), f2i(1.0), f2i(32.0), f2i(1.0)]
    rng = np.random.default_rng(7)
    qc, kc, vc = (dev(rng.normal(0, 1, (1, h, D)).astype(np.float32)) for h in (H, HK, HK))
    pos = dev(np.array([j0], np.int32))
    qd, kr = torch.zeros_like(qc), torch.zeros_like(kc)
    kcache16 = torch.zeros((n_ctx, HK * D), dtype=torch.float16, device="cuda")
    kcache8 = torch.zeros((n_ctx, HK * HB), dtype=torch.uint8, device="cuda")
    vcache = torch.zeros((HK * D, n_ctx), dtype=torch.float16, device="cuda")
    tq, tqd = T(F32, [D, H, 1], data=qc.data_ptr()), T(F32, [D, H, 1], data=qd.data_ptr(), op_params=rope)
    tk, tkr = T(F32, [D, HK, 1], data=kc.data_ptr()), T(F32, [D, HK, 1], data=kr.data_ptr(), op_params=rope)
    tpos = T(I32, [1], data=pos.data_ptr())
    tkd16 = T(F16, [D, HK, 1], data=kcache16.data_ptr() + j0 * HK * D * 2)
    tkd8 = T(Q8_0, [HK * D], nb=[34, HK * HB, HK * HB, HK * HB], data=kcache8.data_ptr() + j0 * HK * HB)
    tv = T(F32, [1, HK * D], nb=[HK * D * 4, 4, HK * D * 4, HK * D * 4], data=vc.data_ptr())
    tvd = T(F16, [1, HK * D], nb=[2, n_ctx * 2, n_ctx * HK * D * 2, n_ctx * HK * D * 2], data=vcache.data_ptr() + j0 * 2)
    store = lib.lib.qmm_rope_kv_store

    def f16_store():
        lib._chk(store(lib.ctx, r(tq), r(tpos), None, r(tqd), r(tk), r(tkd16), r(tv), r(tvd), lib._stream()))

    def q8_store():
        lib._chk(store(lib.ctx, r(tq), r(tpos), None, r(tqd), None, None, r(tv), r(tvd), lib._stream()))
        lib.op(capi.OP_ROPE, tkr, tk, tpos)
        lib.op(capi.OP_CPY, tkd8, tkr)

    runs = [(f16_store, []), (q8_store, [])]
    l8 = lib.trace(q8_store)
    us = timed(runs, a.windows, a.launches)
    lines.append("# the store of one token (rope(q), rope(k) -> K cache, v -> V cache):")
    lines.append(f"store          1 {'':>6}  {'qmm_rope_kv_store(q, k, v): 1 launch':<48} {us[0]:>7.1f}   {'qmm_rope_kv_store(q, v)+' + '+'.join(l8):<56} {us[1]:>7.1f}  {us[1] / us[0]:>5.2f}")
    print(lines[-1], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
