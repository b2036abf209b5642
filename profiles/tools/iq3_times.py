"""Times of MUL_MAT on IQ3_XXS / IQ3_S weights beside Q3_K and IQ4_XS on the same shapes, all through qmm_mul_mat.  The Q3_K and IQ4_XS
columns may be taken from another build of the kernel library (--baseline-lib: the library of the commit a change is compared with), so
they are not the code under test.

    python profiles/tools/iq3_times.py [--baseline-lib PATH] [--out profiles/iq3_times.txt]

The method is profiles/tools/bf16_times.py's.  Mat-vec (N = 1): weight bytes / launch time; each window walks through copies of the
matrix that add up to more than 600 MB, so the weights come from HBM and not from the 256 MiB last-level cache; launch gaps included.
Prompt (N = 512): 2 M K N flop / launch time on one copy, activation prep included, default precision (f16 on Q8 activations).  Per
shape: a warm-up pass, then `--windows` windows of back-to-back launches between two device events, the four variants alternating window
by window; the figure is the median window, the spread its (max - min) / median.

The two grids come from the reference's dequantizer when oracle/_ref is there (tests/iq3_refs.py); otherwise a random table of valid
bytes stands in, which costs the kernels the same."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from ggml_hexagon_amd import capi, synth  # noqa: E402

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]          # (M, K)
WORKING_SET = 600e6
NEW = [(capi.IQ3_XXS, "IQ3_XXS"), (capi.IQ3_S, "IQ3_S")]
OLD = [(capi.Q3_K, "Q3_K"), (capi.IQ4_XS, "IQ4_XS")]


def open_lib(path):
    if path is None:
        return capi.Qmm(0)
    orig = capi._build.build_qmm
    capi._build.build_qmm = lambda force=False: Path(path)
    try:
        return capi.Qmm(0)
    finally:
        capi._build.build_qmm = orig


def codebooks():
    from oracle.pyoracle import ref_available
    if ref_available():
        import iq3_refs
        ref = iq3_refs.Iq3Ref()
        return {t: ref.codebook(t) for t, _ in NEW}, "the reference's grids"
    rng = np.random.default_rng(0)
    return {t: rng.integers(1, 128, 4 * n, dtype=np.uint8).view(np.uint32) for t, n in ((capi.IQ3_XXS, 256), (capi.IQ3_S, 512))}, "random tables of valid bytes"


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "iq3_times.txt"))
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    new = open_lib(None)
    old = open_lib(a.baseline_lib) if a.baseline_lib else new
    books, where = codebooks()
    for t, grid in books.items():
        new.set_codebook(t, grid)
    variants = [(new, t, name) for t, name in NEW] + [(old, t, name) for t, name in OLD]
    lines = [f"# median of {a.windows} windows, spread = (max - min) / median of the windows (profiles/tools/iq3_times.py)",
             f"# IQ3_XXS, IQ3_S: this library, {where}, read from the device table; Q3_K, IQ4_XS: {'baseline library' if a.baseline_lib else 'this library'}",
             f"# mat-vec, N = 1: {a.launches} launches per window over copies of the matrix that exceed the last-level cache; GB/s = weight bytes / launch time",
             "#     M      K  type     launch                               us    GB/s  spread  GB/s : IQ4_XS GB/s"]
    for m, k in SHAPES:
        x = torch.from_numpy(np.random.default_rng(2).standard_normal((1, k)).astype(np.float32)).cuda()
        out = torch.zeros((1, m), device="cuda")
        runs, meta, keep = [], [], []
        for q, t, name in variants:
            w = synth.synth_weights(t, m, k, seed=1)
            wd = torch.from_numpy(w).cuda()
            copies = [wd] + [wd.clone() for _ in range(int(WORKING_SET // w.nbytes))]
            keep.append(copies)
            label = q.trace(lambda: q.mul_mat(t, copies[0], k, x, out=out))
            call = (lambda q, t, copies: lambda i: q.mul_mat(t, copies[i % len(copies)], k, x, out=out))(q, t, copies)
            for i in range(len(copies)):
                call(i)
            runs.append((call, []))
            meta.append((name, "+".join(label), w.nbytes))
        torch.cuda.synchronize()
        res = windows(runs, a.windows, a.launches)
        gbs = [nb / us / 1e3 for (us, _), (_, _, nb) in zip(res, meta)]
        for (us, sp), (name, label, nb), gb in zip(res, meta, gbs):
            lines.append(f"{m:>7} {k:>6}  {name:<8} {label:<32} {us:>7.1f} {gb:>7.0f}  {sp:>5.1%}  {gb / gbs[-1]:.2f}")
            print(lines[-1], flush=True)
        del keep, runs
        torch.cuda.empty_cache()
    n = 512
    lines += [f"# prompt, N = {n}: {max(a.launches // 5, 10)} launches per window on one copy, activation prep included; TFLOP/s = 2 M K N / launch time",
              "#     M      K  type     launches                                                  us  TFLOP/s  spread  : IQ4_XS"]
    for m, k in SHAPES:
        x = torch.from_numpy(np.random.default_rng(2).standard_normal((n, k)).astype(np.float32)).cuda()
        runs, meta, keep = [], [], []
        for q, t, name in variants:
            wd = torch.from_numpy(synth.synth_weights(t, m, k, seed=1)).cuda()
            out = torch.zeros((n, m), device="cuda")
            keep.append((wd, out))
            label = q.trace(lambda: q.mul_mat(t, wd, k, x, out=out))
            call = (lambda q, t, wd, out: lambda i: q.mul_mat(t, wd, k, x, out=out))(q, t, wd, out)
            for i in range(5):
                call(i)
            runs.append((call, []))
            meta.append((name, "+".join(label)))
        torch.cuda.synchronize()
        res = windows(runs, a.windows, max(a.launches // 5, 10))
        tf = [2.0 * m * k * n / us / 1e6 for us, _ in res]
        for (us, sp), (name, label), v in zip(res, meta, tf):
            lines.append(f"{m:>7} {k:>6}  {name:<8} {label:<52} {us:>7.1f} {v:>8.1f}  {sp:>5.1%}  {v / tf[-1]:.2f}")
            print(lines[-1], flush=True)
        del keep, runs
        torch.cuda.empty_cache()
    new.synchronize()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
