"""Times of MUL_MAT on TQ1_0 / TQ2_0 weights beside IQ1_S and Q2_K on the llama3-8b shapes, all four from this build of the kernel
library through qmm_mul_mat.

    python profiles/tools/tq_times.py [--out profiles/tq_times.txt]

The method is profiles/tools/iq1_times.py's.  Mat-vec (N = 1): weight bytes / launch time; each window walks through copies of the
matrix that add up to more than 600 MB, so the weights come from HBM and not from the 256 MiB last-level cache; launch gaps included.
Prompt (N = 512): 2 M K N flop / launch time on one copy, activation prep included, default precision (f16 on Q8 activations).  Per
shape: a warm-up pass, then `--windows` windows of back-to-back launches between two device events, the four variants alternating window
by window; the figure is the median window, the spread its (max - min) / median.  Behind every shape: the time ratios the formats are
compared by (TQ2_0 : Q2_K at 66 against 84 bytes per block, TQ1_0 : IQ1_S at 54 against 50, TQ1_0 : TQ2_0 at 54 against 66).

IQ1_S reads its grid from the device table: the reference's when oracle/_ref is there, random valid bytes otherwise (the same cost)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from ggml_hexagon_amd import capi, synth  # noqa: E402
from iq1_times import codebooks  # noqa: E402
from iq3_times import windows  # noqa: E402

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]          # (M, K)
WORKING_SET = 600e6
TYPES = [(capi.TQ1_0, "TQ1_0"), (capi.TQ2_0, "TQ2_0"), (capi.IQ1_S, "IQ1_S"), (capi.Q2_K, "Q2_K")]
RATIOS = [("TQ2_0", "Q2_K"), ("TQ1_0", "IQ1_S"), ("TQ1_0", "TQ2_0")]


def ratio_line(m, k, us):
    """us: {name: microseconds}"""
    return f"#   {m} x {k} time ratios: " + ", ".join(f"{a} : {b} = {us[a] / us[b]:.2f} (bytes {synth.TYPE_SIZE[getattr(capi, a)] / synth.TYPE_SIZE[getattr(capi, b)]:.2f})" for a, b in RATIOS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tq_times.txt"))
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    q = capi.Qmm(0)
    books, where = codebooks()
    q.set_codebook(capi.IQ1_S, books[capi.IQ1_S])
    lines = [f"# median of {a.windows} windows, spread = (max - min) / median of the windows (profiles/tools/tq_times.py)",
             f"# all four types from one build of the library; IQ1_S on {where}, read from the device table",
             f"# mat-vec, N = 1: {a.launches} launches per window over copies of the matrix that exceed the last-level cache; GB/s = weight bytes / launch time",
             "#     M      K  type     launch                               us    GB/s  spread  GB/s : Q2_K GB/s"]
    for m, k in SHAPES:
        x = torch.from_numpy(np.random.default_rng(2).standard_normal((1, k)).astype(np.float32)).cuda()
        out = torch.zeros((1, m), device="cuda")
        runs, meta, keep = [], [], []
        for t, name in TYPES:
            w = synth.synth_weights(t, m, k, seed=1)
            wd = torch.from_numpy(w).cuda()
            copies = [wd] + [wd.clone() for _ in range(int(WORKING_SET // w.nbytes))]
            keep.append(copies)
            label = q.trace(lambda: q.mul_mat(t, copies[0], k, x, out=out))
            call = (lambda t, copies: lambda i: q.mul_mat(t, copies[i % len(copies)], k, x, out=out))(t, copies)
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
        lines.append(ratio_line(m, k, {name: us for (us, _), (name, _, _) in zip(res, meta)}))
        print(lines[-1], flush=True)
        del keep, runs
        torch.cuda.empty_cache()
    n = 512
    lines += [f"# prompt, N = {n}: {max(a.launches // 5, 10)} launches per window on one copy, activation prep included; TFLOP/s = 2 M K N / launch time",
              "#     M      K  type     launches                                                  us  TFLOP/s  spread  : Q2_K"]
    for m, k in SHAPES:
        x = torch.from_numpy(np.random.default_rng(2).standard_normal((n, k)).astype(np.float32)).cuda()
        runs, meta, keep = [], [], []
        for t, name in TYPES:
            wd = torch.from_numpy(synth.synth_weights(t, m, k, seed=1)).cuda()
            out = torch.zeros((n, m), device="cuda")
            keep.append((wd, out))
            label = q.trace(lambda: q.mul_mat(t, wd, k, x, out=out))
            call = (lambda t, wd, out: lambda i: q.mul_mat(t, wd, k, x, out=out))(t, wd, out)
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
        lines.append(ratio_line(m, k, {name: us for (us, _), (name, _) in zip(res, meta)}))
        print(lines[-1], flush=True)
        del keep, runs
        torch.cuda.empty_cache()
    q.synchronize()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
