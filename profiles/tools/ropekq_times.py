"""Times of a layer's rope and cache stores on a quantized K cache: the three launches the library had (qmm_rope_kv_store(q, v), ROPE(k),
CPY f32 -> type) against the one launch of qmm_rope_kq_store (csrc/qmm_ropekq.hiph), beside the F16 cache's one launch
(qmm_rope_kv_store(q, k, v)), all from one library through the C-ABI of include/ggml_mi355x_ops.h.

    python profiles/tools/ropekq_times.py [--baseline-lib PATH] [--out profiles/ropekq_store_times.txt]

--baseline-lib: another build of the kernel library (the parent commit's, which has no qmm_rope_kq_store), loaded beside this one: its F16
launch and its three launches per type join the same alternation, in the same process, so that the two builds' columns can be compared.

llama3-8b's heads (H = 32, H_kv = 8, D = 128), one token and a batch of 512.  Per batch size: 20 warm-up calls per variant, then 15 windows of
200 back-to-back calls between two device events, the eleven variants (seventeen with a baseline library) alternating window by window; the figure is the median window / 200
(us per call, launch gaps included; operands of these sizes stay in the caches)."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from ggml_hexagon_amd import capi  # noqa: E402

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, I32 = 0, 1, 2, 3, 6, 7, 8, 26
H, HK, D = 32, 8, 128
BLOCK = {Q8_0: 34, Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24}
NAMES = {Q8_0: "q8_0", Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f2i(x):
    return int(np.float32(x).view(np.int32))


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


def open_lib(path):
    """a context on the kernel library at `path` (None: this tree's)"""
    if path is None:
        return capi.Qmm(0)
    orig = capi._build.build_qmm
    capi._build.build_qmm = lambda force=False: Path(path)
    try:
        return capi.Qmm(0)
    finally:
        capi._build.build_qmm = orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ropekq_store_times.txt"))
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = open_lib(None)
    base = open_lib(a.baseline_lib) if a.baseline_lib else None
    T, r = capi.QmmTensor.make, capi.C.byref
    lines = [f"# us per call, median of {a.windows} windows of {a.launches} calls (profiles/tools/ropekq_times.py); H={H} H_kv={HK} D={D}",
             "# the store of a batch (rope(q), rope(k) -> K cache, v -> V cache)",
             "# library: this = the tree's build" + (", base = the baseline library (--baseline-lib)" if base else ""),
             "#   N  K cache  lib   launch(es)                                                                      us  / F16  one / three"]
    n_ctx, j0 = 4096, 1000
    rope = [0, D, 0, 0, 8192, f2i(500000.0), f2i(1.0), f2i(0.0), f2i(1.0), f2i(32.0), f2i(1.0)]
    for n in (1, 512):
        rng = np.random.default_rng(7 + n)
        qc, kc, vc = (dev(rng.normal(0, 1, (n, h, D)).astype(np.float32)) for h in (H, HK, HK))
        pos = dev(np.arange(j0, j0 + n, dtype=np.int32))
        qd, kr = torch.zeros_like(qc), torch.zeros_like(kc)
        kcache16 = torch.zeros((n_ctx, HK * D), dtype=torch.float16, device="cuda")
        vcache = torch.zeros((HK * D, n_ctx), dtype=torch.float16, device="cuda")
        tq, tqd = T(F32, [D, H, n], data=qc.data_ptr()), T(F32, [D, H, n], data=qd.data_ptr(), op_params=rope)
        tk, tkr = T(F32, [D, HK, n], data=kc.data_ptr()), T(F32, [D, HK, n], data=kr.data_ptr(), op_params=rope)
        tpos = T(I32, [n], data=pos.data_ptr())
        tkd16 = T(F16, [D, HK, n], data=kcache16.data_ptr() + j0 * HK * D * 2)
        tv = T(F32, [n, HK * D], nb=[HK * D * 4, 4, n * HK * D * 4, n * HK * D * 4], data=vc.data_ptr())
        tvd = T(F16, [n, HK * D], nb=[2, n_ctx * 2, n_ctx * HK * D * 2, n_ctx * HK * D * 2], data=vcache.data_ptr() + j0 * 2)
        store_q = lib.lib.qmm_rope_kq_store

        def f16_store(l):
            return lambda: l._chk(l.lib.qmm_rope_kv_store(l.ctx, r(tq), r(tpos), None, r(tqd), r(tk), r(tkd16), r(tv), r(tvd), l._stream()))

        def three(l, tkd):
            def run():
                l._chk(l.lib.qmm_rope_kv_store(l.ctx, r(tq), r(tpos), None, r(tqd), None, None, r(tv), r(tvd), l._stream()))
                l.op(capi.OP_ROPE, tkr, tk, tpos)
                l.op(capi.OP_CPY, tkd, tkr)
            return run

        def one(tkd):
            return lambda: lib._chk(store_q(lib.ctx, r(tq), r(tpos), None, r(tqd), r(tk), r(tkd), r(tv), r(tvd), lib._stream()))

        # (library, K cache, launches, call, index of the row a ratio is taken against or None)
        rows = [("this", "f16", "qmm_rope_kv_store(q, k, v): 1 launch", f16_store(lib), None)]
        if base:
            rows.append(("base", "f16", "qmm_rope_kv_store(q, k, v): 1 launch", f16_store(base), None))
        keep = []
        for kt in BLOCK:
            hb = D // 32 * BLOCK[kt]
            row = HK * hb
            caches = [torch.zeros((n_ctx, row), dtype=torch.uint8, device="cuda") for _ in range(3)]     # three launches / one launch / the baseline's three
            keep.append(caches)
            tkds = [T(kt, [D, HK, n], nb=[BLOCK[kt], hb, row, row * n], data=c.data_ptr() + j0 * row) for c in caches]
            assert lib.lib.qmm_rope_kq_store_supported(r(tq), r(tpos), None, r(tqd), r(tk), r(tkds[1]), r(tv), r(tvd)) == 1
            variants = [(lib, "this", three(lib, tkds[0])), (lib, "this", one(tkds[1]))] + ([(base, "base", three(base, tkds[2]))] if base else [])
            first = len(rows)
            for l, where, call in variants:
                traced = l.trace(call)
                rows.append((where, NAMES[kt], ("qmm_rope_kv_store(q, v)+" if len(traced) == 2 else "") + "+".join(traced), call, first if len(traced) == 1 else None))
            torch.cuda.synchronize()
            for c in caches[1:3 if base else 2]:                                                         # the same bytes (tests/test_gpu_rope_kq.py), and bytes at all
                assert caches[0][j0:j0 + n].any() and torch.equal(caches[0], c)
        runs = [(call, []) for _, _, _, call, _ in rows]
        us = timed(runs, a.windows, a.launches)
        for i, (where, kname, name, _, against) in enumerate(rows):
            ratio = f"{us[i] / us[against]:>6.2f}" if against is not None else ""
            lines.append(f"{n:>5}  {kname:<7}  {where:<4}  {name:<78} {us[i]:>7.1f}  {us[i] / us[0]:>5.2f}  {ratio}")
            print(lines[-1], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
