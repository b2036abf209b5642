"""shared test-data builders"""
import numpy as np


def q8_K_tie_rows(n_rows: int, k: int, seed: int = 0) -> np.ndarray:
    """Activation rows built to sit on the double-rounding edge of quantize_row_q8_K_ref
    (ggml/src/ggml-quants.c:2479-2516): elements x for which  f32(iscale*x)  is EXACTLY a half-integer
    while the unrounded product is not.  The reference rounds the product to f32 first and then adds the
    12582912.f magic (nearest_int, ggml-quants.c:372-377), so these land on ties-to-even; a fused
    multiply-add implementation gets a different int8 for about half of them."""
    f32 = np.float32
    rng = np.random.default_rng(seed)
    out = rng.uniform(-0.2, 0.2, (n_rows, k)).astype(f32)
    for r in range(n_rows):
        for b in range(k // 256):
            blk = out[r, b * 256:(b + 1) * 256]
            m = f32(rng.uniform(0.9, 1.0) * rng.choice([-1.0, 1.0]))
            blk[0] = m
            isc = f32(-127.0) / m
            pos = 1
            for h in rng.permutation(np.arange(-60, 60)):
                target = f32(h + 0.5)
                x0 = f32(target / isc)
                cand = x0
                for _ in range(200):
                    if f32(isc * cand) == target and float(isc) * float(cand) != float(target):
                        blk[pos] = cand
                        pos += 1
                        break
                    cand = np.nextafter(cand, f32(np.inf) if rng.random() < 0.5 else f32(-np.inf))
                if pos >= 200:
                    break
    return out


def q8_1_sum_tie_rows(n_rows: int, k: int, seed: int = 0) -> np.ndarray:
    """Activation rows whose every 32-block sits on the double-rounding edge of the Q8_1 block sum (quantize_row_q8_1_ref,
    ggml-quants.c:220-252): s = f16(f32(sum * d)) with the f32 d = amax / 127.  In these blocks f32(sum * d) is EXACTLY halfway between two
    f16 values while the unrounded product is not, so rounding the exact product to f16 in one step (an f32 x f32 -> f16 multiply) lands on
    the other neighbour.  Blocks are drawn at random and kept when a float32 / float64 model of the quantizer says so; what the block sum
    has to be comes from the oracle, not from this model."""
    f32, f64 = np.float32, np.float64
    rng = np.random.default_rng(seed)
    need, kept = n_rows * (k // 32), []
    while sum(len(b) for b in kept) < need:
        x = rng.uniform(-1, 1, (200000, 32)).astype(f32)
        d = (np.abs(x).max(1) / f32(127.0)).astype(f32)
        prod = (x * (f32(1.0) / d)[:, None]).astype(f32).astype(f64)
        q = np.trunc(prod + np.copysign(0.5, prod))                            # roundf: halves away from zero
        total = q.sum(1)
        twice = (total.astype(f32) * d).astype(f32).astype(np.float16)         # the reference: to f32, then to f16
        once = (total * d.astype(f64)).astype(np.float16)                      # the exact product (it fits a double) to f16
        kept.append(x[twice != once])
    return np.concatenate(kept)[:need].reshape(n_rows, k)
