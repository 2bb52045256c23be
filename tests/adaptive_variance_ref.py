"""Host restatement of the variance-driven stopping rule (rt_amd.h, rt_render_adaptive_variance) in float64: the pixel
error from (accumulator, moment), the block error as the mean over a block's in-frame pixels, and the round simulation
given each round's cumulative state.  pixel_error_f32 is the same formula in binary32 and in the kernel's operation order,
for comparing the device's pixel errors with its own accumulator and moments to a few ulp."""
import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])
LUM32 = np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)


def pixel_error(accum, m2):
    """(H, W, 4) linear sums with the sample count in channel 3, (H, W) merged moments → (H, W) float64:
    e = sqrt(M2 / (n (n - 1))) / sqrt(L), L = l(accum.rgb / n); 0 where n < 2, L <= 0 or M2 <= 0."""
    accum = np.asarray(accum, dtype=np.float64)
    m2 = np.asarray(m2, dtype=np.float64)
    n = accum[..., 3]
    two = n >= 2
    lum = (accum[..., :3] / np.where(n > 0, n, 1.0)[..., None]) @ LUM
    ok = two & (lum > 0) & (m2 > 0)
    var = np.where(ok, m2, 0.0) / np.where(two, n * (n - 1.0), 1.0)
    return np.where(ok, np.sqrt(var) / np.sqrt(np.where(ok, lum, 1.0)), 0.0)


def pixel_error_f32(accum, m2):
    """pixel_error in binary32, operation by operation as the merge kernel evaluates it (no contraction)."""
    a = np.asarray(accum, dtype=np.float32)
    m2 = np.asarray(m2, dtype=np.float32)
    n = a[..., 3]
    one = np.float32(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r, g, b = a[..., 0] / n, a[..., 1] / n, a[..., 2] / n
        lum = (LUM32[0] * r + LUM32[1] * g) + LUM32[2] * b
        ok = (n >= 2) & (lum > 0) & (m2 > 0)
        e = np.sqrt(np.where(ok, m2, one) / np.where(ok, n * (n - one), one)) / np.sqrt(np.where(ok, lum, one))
    out = np.where(ok, e, np.float32(0)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def block_error(e, block_w, block_h):
    """(H, W) pixel errors → ceil(H/bh) x ceil(W/bw) float64: the mean over each block's in-frame pixels only."""
    e = np.asarray(e, dtype=np.float64)
    h, w = e.shape
    by, bx = -(-h // block_h), -(-w // block_w)
    s = np.zeros((by * block_h, bx * block_w))
    c = np.zeros((by * block_h, bx * block_w))
    s[:h, :w] = e
    c[:h, :w] = 1.0
    return s.reshape(by, block_h, bx, block_w).sum(axis=(1, 3)) / c.reshape(by, block_h, bx, block_w).sum(axis=(1, 3))


def m2_two_pass(lum, n):
    """(H, W, N) sample luminances → (H, W) float64: the centred second moment of each pixel's first n samples."""
    l = np.asarray(lum, dtype=np.float64)[..., :n]
    return ((l - l.mean(axis=-1, keepdims=True)) ** 2).sum(axis=-1)


def round_counts(batch, max_spp):
    """Samples every pixel of an active block holds after round 0, 1, ..."""
    return [min((k + 1) * batch, max_spp) for k in range(-(-max_spp // batch))]


def block_errors_per_round(accs, lum, batch, max_spp, block_w, block_h):
    """accs[k]: the fixed sequence's accumulator after round k (H, W, 4); lum: (H, W, >= max_spp) sample luminances
    → per round the block errors a block still traced in that round has after it."""
    return [block_error(pixel_error(accs[k], m2_two_pass(lum, c)), block_w, block_h)
            for k, c in enumerate(round_counts(batch, max_spp))]


def simulate(block_errs, batch, min_spp, max_spp, threshold):
    """The stopping rule on per-round block errors (block_errs[k]: all blocks' errors after round k, had they been traced)
    → (stop round per block, final error per block, blocks at max_spp unconverged, rounds).  A block stays active while its
    count < min_spp, or while (threshold == 0 or error >= threshold) and count < max_spp; decisions from round 0 on."""
    counts = round_counts(batch, max_spp)
    shape = np.asarray(block_errs[0]).shape
    active = np.ones(shape, bool)
    stop = np.full(shape, -1, dtype=np.int64)
    final = np.zeros(shape)
    at_max = 0
    rounds = 0
    for k, c in enumerate(counts):
        if not active.any():
            break
        rounds += 1
        e = np.asarray(block_errs[k], dtype=np.float64)
        final = np.where(active, e, final)
        unconverged = np.full(shape, True) if threshold == 0 else ~(e < threshold)
        nxt = active & (c < max_spp) & ((c < min_spp) | unconverged)
        stopped = active & ~nxt
        stop[stopped] = k
        at_max += int((stopped & (c >= max_spp) & unconverged).sum())
        active = nxt
    return stop, final, at_max, rounds


def middle_threshold(errs):
    """The midpoint of the two middle positive values: a threshold no block error equals (the exact median of an even
    count is this midpoint, of an odd count an element of the set — then the midpoint of it and its lower neighbour)."""
    e = np.sort(np.asarray(errs, dtype=np.float64).reshape(-1))
    e = e[e > 0]
    assert len(e) >= 2
    m = len(e) // 2
    return float(0.5 * (e[m - 1] + e[m]))


def percentile_threshold(errs, q):
    """The midpoint of the two positive values around the q-th percentile (same reason)."""
    e = np.sort(np.asarray(errs, dtype=np.float64).reshape(-1))
    e = e[e > 0]
    assert len(e) >= 2
    m = min(max(int(len(e) * q / 100.0), 1), len(e) - 1)
    return float(0.5 * (e[m - 1] + e[m]))
