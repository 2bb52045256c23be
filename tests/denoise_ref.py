"""Host restatement of the edge-avoiding à-trous denoiser exactly as include/rt_amd.h states it (rt_denoise), in
float64 after the float32 division c0 = accum.rgb / accum.w.  Shared by tests/test_denoise_host.py and
tests/test_gpu_denoise.py."""
import numpy as np

H5 = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])


def inv_sq(sigma, i=0):
    """1 / (sigma 2^-i)^2 as rt_denoise passes it to the kernel (float32; +inf → 0, held at FLT_MAX)."""
    if np.isinf(sigma):
        return 0.0
    sd = float(np.float32(sigma)) * 2.0 ** -i
    return float(np.float32(min(1.0 / (sd * sd), float(np.finfo(np.float32).max))))


def initial_colour(accum):
    """c0 = accum.rgb / accum.w in float32, 0 where accum.w == 0 → (H, W, 3) float64."""
    accum = np.asarray(accum, dtype=np.float32)
    w = accum[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(w > 0, accum[..., :3] / np.where(w > 0, w, np.float32(1)), np.float32(0))
    return c.astype(np.float64)


def atrous_linear(accum, normal, position, albedo, hit, obj, iterations=5, sigma_color=np.inf, sigma_normal=np.inf,
                  sigma_position=np.inf, sigma_albedo=np.inf, split_objects=True):
    """c^L of the header's iteration, linear, (H, W, 3) float64.  normal / position / albedo: (H, W, 3); hit: (H, W)
    bool; obj: (H, W) uint32 object ids."""
    c = initial_colour(accum)
    h, w = c.shape[:2]
    guides = [np.asarray(g, dtype=np.float32).astype(np.float64) for g in (normal, position, albedo)]
    hit = np.asarray(hit, dtype=bool)
    obj = np.asarray(obj, dtype=np.uint32)
    inv_g = [inv_sq(sigma_normal), inv_sq(sigma_position), inv_sq(sigma_albedo)]
    ys, xs = np.mgrid[0:h, 0:w]
    for i in range(iterations):
        s = 1 << i
        inv_c = inv_sq(sigma_color, i)
        num = np.zeros_like(c)
        den = np.zeros((h, w))
        for dy in range(-2, 3):           # dy outer, dx inner
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)     # taps outside the frame are skipped
                qy, qx = np.where(ok, qy, 0), np.where(ok, qx, 0)
                cq = c[qy, qx]
                z = inv_c * ((c - cq) ** 2).sum(-1) if inv_c else np.zeros((h, w))
                for g, inv in zip(guides, inv_g):
                    if inv:
                        z = z + inv * ((g - g[qy, qx]) ** 2).sum(-1)
                wt = H5[dx + 2] * H5[dy + 2] * np.exp(-z)
                same = hit == hit[qy, qx]
                if split_objects:
                    same &= obj == obj[qy, qx]
                wt = np.where(ok & same, wt, 0.0)
                num += wt[..., None] * cq
                den += wt
        c = num / den[..., None]
    return c


def atrous(accum, feats, **kw):
    """The header's output: (H, W, 4) RGBA (sqrt(c^L), 1) where accum.w > 0, else 0; `feats` is
    RayTracer.features()'s dict."""
    lin = atrous_linear(accum, feats["normal"], feats["position"], feats["albedo"], feats["hit"], feats["object"], **kw)
    out = np.zeros(lin.shape[:2] + (4,))
    has = np.asarray(accum)[..., 3] > 0
    out[has, :3] = np.sqrt(lin[has])
    out[has, 3] = 1.0
    return out


def b3_blur(img, iterations):
    """The plain B3-spline à-trous blur, computed independently: at step s a direct 5x5 convolution with the kernel
    h (x) h dilated by s, out-of-frame taps skipped and the weights renormalised."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape[:2]
    for i in range(iterations):
        s = 1 << i
        k = np.outer(H5, H5)
        pad = 2 * s
        P = np.zeros((h + 2 * pad, w + 2 * pad) + img.shape[2:])
        M = np.zeros((h + 2 * pad, w + 2 * pad))
        P[pad:pad + h, pad:pad + w] = img
        M[pad:pad + h, pad:pad + w] = 1.0
        num = np.zeros_like(img)
        den = np.zeros((h, w))
        for a in range(5):
            for b in range(5):
                oy, ox = pad + (a - 2) * s, pad + (b - 2) * s
                num += k[a, b] * (P[oy:oy + h, ox:ox + w] * M[oy:oy + h, ox:ox + w][..., None])
                den += k[a, b] * M[oy:oy + h, ox:ox + w]
        img = num / den[..., None]
    return img
