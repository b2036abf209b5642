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


STABLE_MARGIN = 2.0 ** -20                   # 8 f32 ulps: two f32 evaluations of rms_norm * w differ by a few
STABLE_MAX_REDRAWS = 256
Q8_0, Q8_1, Q8_K = 8, 9, 15                  # the activation formats (ggml type ids)


def rms_norm_f64(x, w, eps):
    """rms_norm(x, eps) * w of every row, in float64"""
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * np.asarray(w, np.float64)


def rms_norm_f32(x, w, eps):
    """the numpy-normed f32 rows the references of the norm-fold tests are fed (test_gpu_matvec_head.py::rms_norm): the scale from a
    float64 mean, the two products in f32 in the kernel's order"""
    x64 = x.astype(np.float64)
    return (x * (1.0 / np.sqrt((x64 * x64).mean(axis=-1, keepdims=True) + eps)).astype(np.float32) * w).astype(np.float32)


def _same_f16(v):
    """per element: v (float64) rounds to the same f16 at both ends of the margin"""
    return (v * (1 - STABLE_MARGIN)).astype(np.float16) == (v * (1 + STABLE_MARGIN)).astype(np.float16)


def rounding_stable(fmt, xn):
    """whether the quantization of the row xn (float64, the normed row) to `fmt` is the same for every row within a few f32 ulps of it.
    Element condition: every v = xn_i * 127 / amax_block (amax per 256 elements for Q8_K, per 32 for Q8_0 / Q8_1) lies farther than
    |v| * 2^-20 + 1e-9 from a half-integer, and no block is all zero.  Block scale condition (Q8_0 / Q8_1): amax / 127 rounds to the
    same f16 at * (1 - 2^-20) and * (1 + 2^-20).  Two more, found by perturbing rows that met those two: Q8_1's s is f16(sum(q) * d) with
    the F32 d = amax / 127 (quantize_row_q8_1_ref), which moves with amax although q and the f16 d do not, so sum(q) * amax / 127 has to
    round to one f16 over the margin as well; and Q8_K's scale takes the SIGN of the first element of largest magnitude, so a block
    whose two largest magnitudes lie within the margin of each other could change every sign of its block (the product is the same, the
    bytes are not)."""
    blk = xn.reshape(-1, 256 if fmt == Q8_K else 32)
    a = np.abs(blk)
    amax = a.max(axis=1, keepdims=True)
    if not (amax > 0).all():
        return False
    v = blk * 127.0 / amax
    if not (np.abs(np.abs(v - np.floor(v)) - 0.5) > np.abs(v) * STABLE_MARGIN + 1e-9).all():
        return False
    if fmt == Q8_K:
        second = np.sort(a, axis=1)[:, -2:-1]
        return bool((second < amax * (1 - 2 * STABLE_MARGIN)).all())
    d = amax[:, 0] / 127.0
    if not _same_f16(d).all():
        return False
    return fmt == Q8_0 or bool(_same_f16(np.rint(v).sum(axis=1) * d).all())


def rounding_stable_rows(fmt, n_rows, k, norm_w, eps, seed=0, shape=None):
    """The opposite of q8_K_tie_rows: N(0, 1) rows x [n_rows, k] (f32) whose rms_norm(x, eps) * norm_w quantizes to `fmt` (Q8_K, Q8_0 or
    Q8_1) the same way whatever the last bits of the norm (rounding_stable), so that a kernel that forms the norm in f32 and a reference that
    forms it in numpy hand the same int8 values and block scales to the dot products.  A rejected row is redrawn whole from the same
    generator, up to STABLE_MAX_REDRAWS times (then: RuntimeError; no row is dropped).  shape(r, row), if given, reshapes every draw of row
    r before it is judged (the value edges of the fold tests).  Returns (x, redraws per row)."""
    rng = np.random.default_rng(seed)
    x = np.empty((n_rows, k), np.float32)
    redraws = np.zeros(n_rows, np.int64)
    for r in range(n_rows):
        while True:
            row = rng.normal(0.0, 1.0, k).astype(np.float32)
            if shape is not None:
                row = np.asarray(shape(r, row), np.float32)
            if rounding_stable(fmt, rms_norm_f64(row, norm_w, eps)):
                break
            redraws[r] += 1
            if redraws[r] > STABLE_MAX_REDRAWS:
                raise RuntimeError(f"no rounding-stable row of K = {k} for activation format {fmt} within {STABLE_MAX_REDRAWS} redraws")
        x[r] = row
    return x, redraws


def quantize_stable(fmt, xn):
    """the wire blocks of rounding-stable rows xn (f32 [n, k], what a reference is fed), as the CPU backend's quantizers write them
    (block_q8_0: f16 d, 32 int8; block_q8_1: f16 d, f16 s, 32 int8; block_q8_K: f32 d, 256 int8, 16 int16 sums): uint8 [n, row bytes].
    The int8 values are rint() of the float64 quotient, which is what every rounding mode gives off the half-integers"""
    f32 = np.float32
    xn = np.asarray(xn, f32)
    n, k = xn.shape
    if fmt == Q8_K:
        blk = xn.reshape(n, k // 256, 256)
        peak = np.take_along_axis(blk, np.abs(blk).argmax(axis=2)[..., None], axis=2)          # signed, the first of largest magnitude
        q = np.minimum(np.rint(blk.astype(np.float64) * -127.0 / peak), 127).astype(np.int8)
        iscale = f32(-127.0) / peak.astype(f32)
        out = np.zeros((n, k // 256, 292), np.uint8)
        out[:, :, 0:4] = (f32(1.0) / iscale).astype(f32).view(np.uint8).reshape(n, k // 256, 4)
        out[:, :, 4:260] = q.view(np.uint8)
        out[:, :, 260:292] = q.reshape(n, k // 256, 16, 16).sum(axis=3).astype(np.int16).view(np.uint8).reshape(n, k // 256, 32)
        return out.reshape(n, -1)
    blk = xn.reshape(n, k // 32, 32)
    amax = np.abs(blk).max(axis=2, keepdims=True)
    d = (amax / f32(127.0)).astype(f32)
    q = np.rint(blk.astype(np.float64) * 127.0 / amax).astype(np.int8)
    head = 2 if fmt == Q8_0 else 4
    out = np.zeros((n, k // 32, head + 32), np.uint8)
    out[:, :, 0:2] = d.astype(np.float16).view(np.uint8).reshape(n, k // 32, 2)
    if fmt == Q8_1:
        s = (q.sum(axis=2, keepdims=True).astype(f32) * d).astype(f32)
        out[:, :, 2:4] = s.astype(np.float16).view(np.uint8).reshape(n, k // 32, 2)
    out[:, :, head:] = q.view(np.uint8)
    return out.reshape(n, -1)


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
