"""numpy statements of the sample queue's per-pixel summation (csrc/pt_queue.hpp queue_sums), float32 throughout.

butterfly_lane0  the CONTRACT: lane l of a pixel's g = 1 << group_log2 lanes starts from 0.0f and adds its slots
                 l, l + g, … in that order; then for off = g/2 … 1 every lane adds lane l ^ off's value to its own;
                 lane 0's value is the pixel's sum (what pt_render's group_sum leaves in lane 0).
half_tree_lane0  the same tree without its redundant half: for off = g/2 … 1, for l < off, T(l) = T(l) + T(l + off).
wave_tree        queue_sums_tree AS IMPLEMENTED, a wave of 64 lanes with its registers as arrays of 64: the same pairing
                 of pixels to half-waves and rows, the same swap and row shifts, the same lanes that store.

Shared by tests/test_queue_sums_host.py (the three agree, bit for bit) and tests/test_gpu_queue_sums.py (the device
agrees with the contract)."""
import numpy as np

f32 = np.float32
LANES = np.arange(64)
COUNTS = (1, 2, 3, 5, 8, 16, 17, 24, 32, 33, 63, 64, 65, 128, 200, 512)
QUEUE_SLOTS, QUEUE_MAX_PIXELS = 512, 16     # csrc/rt_context.hpp


def max_pixels(count):
    """The most pixels of `count` samples one wave may own."""
    return min(QUEUE_MAX_PIXELS, QUEUE_SLOTS // count)


def pixel_counts(count):
    """npix of the cases: 1, the largest a wave may own at this count, and one value in between."""
    m = max_pixels(count)
    return sorted({1, (m + 1) // 2 + (1 if m > 4 else 0), m})


def adversarial(npix, count, seed):
    """(npix, count, 3) float32: magnitudes 1e-20 … 1e20 of both signs, with ±0, denormals and — in some pixels —
    infinities mixed in (of one sign or of both, so that some sums are NaN)."""
    r = np.random.RandomState(seed)
    shape = (npix, count, 3)
    with np.errstate(over="ignore", under="ignore"):
        v = (10.0 ** r.uniform(-20, 20, shape) * r.choice([-1.0, 1.0], shape)).astype(f32)
        kind = r.randint(0, 16, shape)
        v[kind == 0] = f32(0.0)
        v[kind == 1] = f32(-0.0)
        den = (r.randint(1, 1 << 23, shape).astype(np.uint32) | (r.randint(0, 2, shape).astype(np.uint32) << 31)).view(f32)
        v[kind == 2] = den[kind == 2]
        v[kind == 3] = (r.uniform(-4, 4, shape)).astype(f32)[kind == 3]          # same-magnitude values: cancellation
        for p in range(npix):
            mode = r.randint(0, 6)
            if mode >= 3:                                                         # half of the pixels keep finite slots
                continue
            n = max(1, count // 8)
            js, cs = r.randint(0, count, n), r.randint(0, 3, n)
            inf = (np.full(n, np.inf), np.full(n, -np.inf), r.choice([np.inf, -np.inf], n))[mode]
            v[p, js, cs] = inf.astype(f32)
    return v


def _lane_sums(vals, g):
    """vals (count, C) → (g, C): lane l's 0.0f + slot l + slot l+g + …"""
    count = len(vals)
    S = np.zeros((g,) + vals.shape[1:], f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, count, g):
            n = min(g, count - k)
            S[:n] = S[:n] + vals[k:k + n]
    return S


def butterfly_lane0(vals, g):
    S = _lane_sums(vals, g)
    off = g >> 1
    with np.errstate(invalid="ignore", over="ignore"):
        while off:
            S = S + S[np.arange(g) ^ off]
            off >>= 1
    return S[0]


def half_tree_lane0(vals, g):
    T = _lane_sums(vals, g)
    off = g >> 1
    with np.errstate(invalid="ignore", over="ignore"):
        while off:
            T[:off] = T[:off] + T[off:2 * off]
            off >>= 1
    return T[0]


# ---- the wave as queue_sums_tree runs it ---------------------------------------------------------------------------
def _queue_lane_sum(slots, p, l, g):
    """queue_lane_sum for all 64 lanes: p, l arrays of 64 → (64, 3); a pixel the wave does not own: zeros, nothing read."""
    npix, count = slots.shape[0], slots.shape[1]
    out = np.zeros((64, 3), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for lane in range(64):
            if p[lane] >= npix:
                continue
            s = np.zeros(3, f32)
            for j in range(int(l[lane]), count, g):
                s = s + slots[p[lane], j]
            out[lane] = s
    return out


def _row_add(v, off):
    """v(i) + v(i + off) within a row of 16 lanes; a lane whose partner lies outside its row adds 0 (DPP row_shl, old = 0)."""
    src = LANES + off
    ok = (src >> 4) == (LANES >> 4)
    t = np.zeros_like(v)
    t[ok] = v[src[ok]]
    with np.errstate(invalid="ignore", over="ignore"):
        return v + t


def _row_pair_add(a, b):
    """v_permlane16_swap exchanges a's odd rows with b's even rows; then one add."""
    a2, b2 = a.copy(), b.copy()
    for r in (1, 3):
        odd, even = slice(16 * r, 16 * r + 16), slice(16 * r - 16, 16 * r)
        a2[odd], b2[even] = b[even], a[odd]
    with np.errstate(invalid="ignore", over="ignore"):
        return a2 + b2


def wave_tree(slots, group_log2):
    """slots (npix, count, 3) → (npix, 3): what the lanes that store add to the accumulator."""
    npix = slots.shape[0]
    gl, g = group_log2, 1 << group_log2
    out = np.full((npix, 3), np.nan, f32)
    stored = np.zeros(npix, bool)
    if gl >= 5:
        half, i, row = LANES >> 5, LANES & 31, LANES >> 4
        for pb in range(0, npix, 4):
            a, b = _queue_lane_sum(slots, pb + half, i, g), _queue_lane_sum(slots, pb + 2 + half, i, g)
            if gl == 6:
                with np.errstate(invalid="ignore", over="ignore"):
                    a = a + _queue_lane_sum(slots, pb + half, i + 32, g)
                    b = b + _queue_lane_sum(slots, pb + 2 + half, i + 32, g)
            s = _row_pair_add(a, b)
            for off in (8, 4, 2, 1):
                s = _row_add(s, off)
            p = pb + ((row & 1) << 1 | row >> 1)
            for lane in LANES[(p < npix) & ((LANES & 15) == 0)]:
                assert not stored[p[lane]]
                out[p[lane]], stored[p[lane]] = s[lane], True
    else:
        ppp = 64 >> gl
        for pb in range(0, npix, ppp):
            p, l = pb + (LANES >> gl), LANES & (g - 1)
            s = _queue_lane_sum(slots, p, l, g)
            for need, off in ((4, 8), (3, 4), (2, 2), (1, 1)):
                if gl >= need:
                    s = _row_add(s, off)
            for lane in LANES[(p < npix) & (l == 0)]:
                assert not stored[p[lane]]
                out[p[lane]], stored[p[lane]] = s[lane], True
    assert stored.all()
    return out


def contract(slots, group_log2):
    """slots (npix, count, 3) → (npix, 3): the butterfly's lane 0, pixel by pixel."""
    return np.stack([butterfly_lane0(slots[p], 1 << group_log2) for p in range(slots.shape[0])])


def same_bits(got, ref):
    """Bit equality; where the contract's sum is a NaN (a pixel whose slots hold +inf and -inf) the other must be a NaN too —
    its payload and sign are the adder's choice (x86 and gfx950 differ in the NaN an invalid operation makes)."""
    got, ref = np.asarray(got, f32), np.asarray(ref, f32)
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))
