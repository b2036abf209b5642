"""Times of MUL_MAT on BF16 weights beside the Q8_0 launch of the same shapes, both through qmm_mul_mat.  The Q8_0 column may be taken from
another build of the kernel library (--baseline-lib: the library of the commit a change is compared with), so it is not the code under test.

    python profiles/tools/bf16_times.py [--baseline-lib PATH] [--out profiles/bf16_times.txt]

Mat-vec (N = 1): weight bytes / launch time.  A 4096 x 4096 matrix is 32 MiB in BF16 and would be served from the 256 MiB last-level
cache if one matrix were launched over and over, so each window walks through copies of the matrix that add up to more than 600 MB, as
the layers of a model do; the figure is HBM bandwidth, launch gaps included.  Prompt (N = 512): 2 M K N flop / launch time on one copy;
the Q8_0 column runs under QMM_PREC_BF16 (the same MFMA with an unpack in front) and counts its activation prep, which the BF16 kernel
does on its way into LDS.  Per shape and variant: a warm-up pass, then `--windows` windows of `--launches` back-to-back launches between
two device events, the two variants alternating window by window; the figure is the median window, the spread its (max - min) / median."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from ggml_hexagon_amd import capi, synth  # noqa: E402

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]          # (M, K)
WORKING_SET = 600e6


def open_lib(path):
    if path is None:
        return capi.Qmm(0)
    orig = capi._build.build_qmm
    capi._build.build_qmm = lambda force=False: Path(path)
    try:
        return capi.Qmm(0)
    finally:
        capi._build.build_qmm = orig


def copies_of(w_np, n):
    w = torch.from_numpy(np.ascontiguousarray(w_np)).cuda()
    return [w] + [w.clone() for _ in range(n - 1)]


def windows(runs, n_windows, launches):
    """runs: list of (call(i), times[]) timed alternately; call(i) issues launch i of a window"""
    for _ in range(n_windows):
        for call, times in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(launches):
                call(i)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1000.0 / launches)
    return [(statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for _, t in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bf16_times.txt"))
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    new = open_lib(None)
    old = open_lib(a.baseline_lib) if a.baseline_lib else new
    base = "baseline library" if a.baseline_lib else "this library"
    lines = [f"# median of {a.windows} windows of {a.launches} launches, spread = (max - min) / median of the windows (profiles/tools/bf16_times.py)",
             f"# BF16: this library; Q8_0: {base}",
             "# mat-vec, N = 1: weight bytes / launch time over copies of the matrix that exceed the last-level cache",
             "#     M      K  BF16 launch                    us    GB/s  spread | Q8_0 launch                      us    GB/s  spread | BF16 GB/s / Q8_0 GB/s"]
    for m, k in SHAPES:
        wb = synth.synth_weights_bf16(m, k, seed=1).view(np.uint8)
        wq = synth.synth_weights(synth.Q8_0, m, k, seed=1)
        cb, cq = copies_of(wb, int(WORKING_SET // wb.nbytes) + 1), copies_of(wq, int(WORKING_SET // wq.nbytes) + 1)
        x = torch.from_numpy(np.random.default_rng(2).standard_normal((1, k)).astype(np.float32)).cuda()
        out = torch.zeros((1, m), device="cuda")
        lb = new.trace(lambda: new.mul_mat(capi.BF16, cb[0], k, x, out=out))
        lq = old.trace(lambda: old.mul_mat(capi.Q8_0, cq[0], k, x, out=out))
        fb = lambda i: new.mul_mat(capi.BF16, cb[i % len(cb)], k, x, out=out)
        fq = lambda i: old.mul_mat(capi.Q8_0, cq[i % len(cq)], k, x, out=out)
        for i in range(max(len(cb), len(cq))):
            fb(i), fq(i)
        torch.cuda.synchronize()
        (ub, sb), (uq, sq) = windows([(fb, []), (fq, [])], a.windows, a.launches)
        gb, gq = wb.nbytes / ub / 1e3, wq.nbytes / uq / 1e3
        lines.append(f"{m:>7} {k:>6}  {'+'.join(lb):<28} {ub:>7.1f} {gb:>7.0f}  {sb:>5.1%} | {'+'.join(lq):<28} {uq:>7.1f} {gq:>7.0f}  {sq:>5.1%} | {gb / gq:.2f}")
        print(lines[-1], flush=True)
        del cb, cq
        torch.cuda.empty_cache()
    lines += ["# prompt, N = 512: 2 M K N flop / launch time (Q8_0 under QMM_PREC_BF16, its activation prep included)",
              "#     M      K  BF16 launch                    us  TFLOP/s  spread | Q8_0 launches                                       us  TFLOP/s  spread | BF16 / Q8_0"]
    old.set_precision(capi.PREC_BF16)
    n = 512
    for m, k in SHAPES:
        wb = torch.from_numpy(synth.synth_weights_bf16(m, k, seed=1).view(np.uint8)).cuda()
        wq = torch.from_numpy(synth.synth_weights(synth.Q8_0, m, k, seed=1)).cuda()
        x = torch.from_numpy(np.random.default_rng(2).standard_normal((n, k)).astype(np.float32)).cuda()
        ob, oq = torch.zeros((n, m), device="cuda"), torch.zeros((n, m), device="cuda")
        lb = new.trace(lambda: new.mul_mat(capi.BF16, wb, k, x, out=ob))
        lq = old.trace(lambda: old.mul_mat(capi.Q8_0, wq, k, x, out=oq))
        fb = lambda i: new.mul_mat(capi.BF16, wb, k, x, out=ob)
        fq = lambda i: old.mul_mat(capi.Q8_0, wq, k, x, out=oq)
        for i in range(5):
            fb(i), fq(i)
        torch.cuda.synchronize()
        (ub, sb), (uq, sq) = windows([(fb, []), (fq, [])], a.windows, max(a.launches // 5, 10))
        tb, tq = 2.0 * m * k * n / ub / 1e6, 2.0 * m * k * n / uq / 1e6
        lines.append(f"{m:>7} {k:>6}  {'+'.join(lb):<28} {ub:>7.1f} {tb:>8.1f}  {sb:>5.1%} | {'+'.join(lq):<48} {uq:>7.1f} {tq:>8.1f}  {sq:>5.1%} | {tb / tq:.2f}")
        print(lines[-1], flush=True)
    old.set_precision(capi.PREC_F16_Q8)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
