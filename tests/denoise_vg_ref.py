"""Host restatement of the variance-guided denoiser exactly as include/rt_amd.h states it (rt_denoise_variance), in
float64 after the float32 division c0 = accum.rgb / accum.w.  The guide sigmas enter as the float32 1/sigma^2
(denoise_ref.inv_sq), sigma_luminance and eps as their float32 values.  Shared by tests/test_denoise_vg_host.py and
tests/test_gpu_denoise_vg.py."""
import numpy as np

from denoise_ref import H5, initial_colour, inv_sq

K3 = np.array([0.25, 0.5, 0.25])
LUM = np.array([0.2126, 0.7152, 0.0722])
EPS = float(np.float32(1e-4))


def luminance(c):
    return c @ LUM


class Guides:
    """g_pq of the header for shifted copies of the frame: normal / position / albedo (H, W, 3), hit (H, W) bool, obj
    (H, W) uint32."""

    def __init__(self, normal, position, albedo, hit, obj, sigma_normal, sigma_position, sigma_albedo, split_objects):
        self.g = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in (normal, position, albedo)]
        self.inv = [inv_sq(sigma_normal), inv_sq(sigma_position), inv_sq(sigma_albedo)]
        self.hit = np.asarray(hit, dtype=bool)
        self.obj = np.asarray(obj, dtype=np.uint32)
        self.split = bool(split_objects)
        self.h, self.w = self.hit.shape
        self.ys, self.xs = np.mgrid[0:self.h, 0:self.w]

    def tap(self, oy, ox):
        """→ (ok, qy, qx, z): the tap q = p + (ox, oy) of every pixel p; ok = inside the frame and key_q == key_p (the
        indices of the others are clamped to 0 and must not be used); z = the guides' summed exponent."""
        qy, qx = self.ys + oy, self.xs + ox
        ok = (qy >= 0) & (qy < self.h) & (qx >= 0) & (qx < self.w)
        qy, qx = np.where(ok, qy, 0), np.where(ok, qx, 0)
        z = np.zeros((self.h, self.w))
        for g, inv in zip(self.g, self.inv):
            if inv:
                z = z + inv * ((g - g[qy, qx]) ** 2).sum(-1)
        same = self.hit == self.hit[qy, qx]
        if self.split:
            same &= self.obj == self.obj[qy, qx]
        return ok & same, qy, qx, z


def variance_estimate(c0, guides):
    """Step 1: v0, the 7x7 guide-weighted two-pass luminance variance → (H, W) float64."""
    l = luminance(c0)
    taps = []
    m0 = np.zeros_like(l)
    m1 = np.zeros_like(l)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            ok, qy, qx, z = guides.tap(dy, dx)
            g = np.where(ok, np.exp(-z), 0.0)
            lq = l[qy, qx]
            taps.append((g, lq))
            m0 += g
            m1 += g * lq
    m = m1 / m0
    m2 = np.zeros_like(l)
    for g, lq in taps:
        m2 += g * (lq - m) ** 2
    return m2 / m0


def unit_blur(v):
    """vt: the 3x3 binomial over the unit neighbours inside the frame, renormalised, no edge stopping."""
    h, w = v.shape
    P = np.zeros((h + 2, w + 2))
    M = np.zeros((h + 2, w + 2))
    P[1:-1, 1:-1] = v
    M[1:-1, 1:-1] = 1.0
    num = np.zeros((h, w))
    den = np.zeros((h, w))
    for a in range(3):
        for b in range(3):
            k = K3[a] * K3[b]
            num += k * P[a:a + h, b:b + w]
            den += k * M[a:a + h, b:b + w]
    return num / den


def filter_linear(accum, normal, position, albedo, hit, obj, iterations=5, sigma_luminance=np.inf, sigma_normal=np.inf,
                  sigma_position=np.inf, sigma_albedo=np.inf, split_objects=True):
    """→ (c(L) (H, W, 3), v0 (H, W), v(L) (H, W)), linear, float64."""
    c = initial_colour(accum)
    guides = Guides(normal, position, albedo, hit, obj, sigma_normal, sigma_position, sigma_albedo, split_objects)
    v0 = variance_estimate(c, guides)
    v = v0
    lum_on = not np.isinf(sigma_luminance)
    sigma_l = float(np.float32(sigma_luminance)) if lum_on else 0.0
    for i in range(iterations):
        s = 1 << i
        l = luminance(c)
        d = sigma_l * np.sqrt(unit_blur(v)) + EPS
        num = np.zeros_like(c)
        numv = np.zeros_like(v)
        den = np.zeros_like(v)
        for dy in range(-2, 3):           # dy outer, dx inner
            for dx in range(-2, 3):
                ok, qy, qx, z = guides.tap(s * dy, s * dx)
                if lum_on:
                    z = z + np.abs(l - l[qy, qx]) / d
                wt = np.where(ok, H5[dx + 2] * H5[dy + 2] * np.exp(-z), 0.0)
                num += wt[..., None] * c[qy, qx]
                numv += wt * wt * v[qy, qx]
                den += wt
        c = num / den[..., None]
        v = numv / den ** 2
    return c, v0, v


def filter_frame(accum, feats, **kw):
    """The header's output: ((H, W, 4) RGBA (sqrt(c(L)), 1) where accum.w > 0, else 0; v0; v(L)); `feats` is
    RayTracer.features()'s dict."""
    lin, v0, vl = filter_linear(accum, feats["normal"], feats["position"], feats["albedo"], feats["hit"],
                                feats["object"], **kw)
    out = np.zeros(lin.shape[:2] + (4,))
    has = np.asarray(accum)[..., 3] > 0
    out[has, :3] = np.sqrt(lin[has])
    out[has, 3] = 1.0
    return out, v0, vl
