"""Times of the FLASH_ATTN_EXT launches (QMM_TENSOR_KV_ROWS: V rows are cache positions, f16 mask) beside the transposed-V launches of the
default path on the same shapes and data, both through the attention ABI.  The transposed-V column may be taken from another build of
the kernel library (--baseline-lib: the library of the commit a change is compared with), so it is not the code under test.

    python profiles/tools/flash_attn_times.py [--baseline-lib PATH] [--lib PATH] [--out profiles/flash_attn_times.txt]

Per shape and variant: 20 warm-up launches, then 15 windows of 200 back-to-back launches between two device events, the two variants
alternating window by window; the figure is the median window / 200 (us per launch, launch gaps included; operands of these sizes stay in
the caches).  H = 32, H_kv = 8, D = 128, llama.cpp's operand layout (strided cache views, permuted q), causal masks."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from ggml_hexagon_amd import capi  # noqa: E402

F32, F16 = 0, 1
H, HK, D = 32, 8, 128
SHAPES = [("prompt", 512, 512), ("prompt", 512, 2048), ("few tokens", 1, 256), ("few tokens", 1, 1024), ("few tokens", 1, 4096)]


def open_lib(path):
    if path is None:
        return capi.Qmm(0)
    orig = capi._build.build_qmm
    capi._build.build_qmm = lambda force=False: Path(path)
    try:
        return capi.Qmm(0)
    finally:
        capi._build.build_qmm = orig


def operands(n_tok, n_kv):
    rng = np.random.default_rng(n_tok + n_kv)
    n_ctx = n_kv + 256
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    q = dev(rng.normal(0, 1, (n_tok, H, D)).astype(np.float32))
    kc = rng.normal(0, 1, (n_ctx, HK, D)).astype(np.float16)
    vc = rng.normal(0, 1, (n_ctx, HK, D)).astype(np.float16)
    rows = (n_tok + 63) // 64 * 64
    m = np.full((rows, n_kv), -np.inf, np.float32)
    for t in range(n_tok):
        m[t, :n_kv - n_tok + t + 1] = 0.0
    k, v_rows, v_t = dev(kc), dev(vc), dev(vc.transpose(1, 2, 0))              # V cache [n_ctx, hk * d] and its transposed form [hk * d, n_ctx]
    m32, m16 = dev(m), dev(m.astype(np.float16))
    outs = [torch.zeros((n_tok, H * D), device="cuda") for _ in range(2)]
    T = capi.QmmTensor.make
    tq = T(F32, [D, n_tok, H], nb=[4, H * D * 4, D * 4, n_tok * H * D * 4], data=q.data_ptr())
    tk = T(F16, [D, n_kv, HK], nb=[2, HK * D * 2, D * 2, n_ctx * HK * D * 2], data=k.data_ptr())
    tvt = T(F16, [n_kv, D, HK], nb=[2, n_ctx * 2, n_ctx * D * 2, n_ctx * D * HK * 2], data=v_t.data_ptr())
    tvr = T(F16, [D, n_kv, HK], nb=[2, HK * D * 2, D * 2, n_ctx * HK * D * 2], data=v_rows.data_ptr(), flags=capi.TENSOR_KV_ROWS)
    old = (tq, tk, tvt, T(F32, [n_kv, rows], data=m32.data_ptr()), T(F32, [H * D, n_tok], data=outs[0].data_ptr()))
    new = (tq, tk, tvr, T(F16, [n_kv, rows], data=m16.data_ptr()), T(F32, [H * D, n_tok], data=outs[1].data_ptr()))
    keep = (q, k, v_rows, v_t, m32, m16)
    return old, new, outs, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--lib", default=None, help="the library whose rows-V launches are timed (default: the tree's)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "flash_attn_times.txt"))
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    new_lib = open_lib(a.lib)
    old_lib = open_lib(a.baseline_lib) if a.baseline_lib else new_lib
    lines = [f"# us per launch, median of {a.windows} windows of {a.launches} launches (profiles/tools/flash_attn_times.py); H={H} H_kv={HK} D={D}",
             f"# transposed V: the default path's launch ({'baseline library' if a.baseline_lib else 'this library'}); rows V: FLASH_ATTN_EXT's launch (this library)",
             "# family      N   n_kv  transposed-V launch(es)                                   us   rows-V launch(es)                                     us  ratio  max|diff|/rms"]
    scale = 1.0 / np.sqrt(D)
    for family, n_tok, n_kv in SHAPES:
        old, new, outs, keep = operands(n_tok, n_kv)
        few = n_tok <= 8
        runs = []
        for lib, ts in ((old_lib, old), (new_lib, new)):
            fn = lib.lib.qmm_attn_decode if few else lib.lib.qmm_attn_prefill
            refs = [capi.C.byref(t) for t in ts]
            call = (lambda lib=lib, fn=fn, refs=refs: lib._chk(fn(lib.ctx, *refs, scale, lib._stream())))
            labels = lib.trace(call)
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            runs.append((call, labels, []))
        for _ in range(a.windows):
            for call, _, times in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    call()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1000.0 / a.launches)
        us = [statistics.median(t) for _, _, t in runs]
        o, n = outs[0].cpu().numpy().astype(np.float64), outs[1].cpu().numpy().astype(np.float64)
        diff = float(np.max(np.abs(o - n)) / np.sqrt(np.mean(o ** 2)))
        lines.append(f"{family:<11} {n_tok:>4} {n_kv:>6}  {'+'.join(runs[0][1]):<52} {us[0]:>7.1f}   {'+'.join(runs[1][1]):<48} {us[1]:>7.1f}  {us[1] / us[0]:>5.2f}  {diff:.1e}")
        print(lines[-1], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
