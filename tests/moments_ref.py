"""Host restatement of the per-pixel sample moments (RT_OPT_MOMENTS, include/rt_amd.h) and of rt_denoise_moments, in
float64: the two-pass centred second moment, the pairwise merge rule, and the variance-guided filter of
tests/denoise_vg_ref.py with its step 1 handed in.  Shared by tests/test_moments_host.py and tests/test_gpu_moments.py."""
import numpy as np

from denoise_ref import H5, initial_colour
from denoise_vg_ref import EPS, LUM, Guides, luminance, unit_blur, variance_estimate

MIN_COUNT = 4   # RT_DENOISE_MOMENTS_MIN_COUNT


def m2_two_pass(samples):
    """(…, n, 3) sample radiances → (…) float64: M2 = sum_j (l(s_j) - mean)^2, the mean taken first."""
    l = np.asarray(samples, dtype=np.float64) @ LUM
    return ((l - l.mean(axis=-1, keepdims=True)) ** 2).sum(axis=-1)


def merge(nA, sumA, m2A, nB, sumB, m2B):
    """The header's merge rule in float64: (nA, SA, M2A) (+) (nB, SB, M2B) → M2."""
    if nA == 0:
        return float(m2B)
    if nB == 0:
        return float(m2A)
    delta = float(np.asarray(sumB, np.float64) @ LUM) / nB - float(np.asarray(sumA, np.float64) @ LUM) / nA
    return float(m2A) + float(m2B) + delta * delta * (nA * nB / (nA + nB))


def tolerance(m2, n, lmax):
    """What a float32 evaluation may deviate from the float64 two-pass M2 of n samples whose largest luminance is lmax:
    1e-4 M2 covers <= 512 float32 additions; e = 1e-6 lmax is 4 x the rounding of l(s) - m in binary32, which enters as
    2 e sqrt(n M2) (the cross term) and n e^2."""
    e = 1e-6 * np.asarray(lmax, dtype=np.float64)
    m2 = np.asarray(m2, dtype=np.float64)
    return 1e-4 * m2 + 2.0 * e * np.sqrt(n * m2) + n * e * e


def measured_v0(m2, n, spatial_v0):
    """Step 1 of rt_denoise_moments: M2 / (n (n - 1)) where n >= MIN_COUNT, the 7x7 estimate elsewhere (n = 0 included)."""
    m2 = np.asarray(m2, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    ok = n >= MIN_COUNT
    return np.where(ok, m2 / np.where(ok, n * (n - 1.0), 1.0), spatial_v0)


def filter_linear_given_v0(accum, v0, normal, position, albedo, hit, obj, iterations=5, sigma_luminance=np.inf,
                           sigma_normal=np.inf, sigma_position=np.inf, sigma_albedo=np.inf, split_objects=True):
    """The loop of denoise_vg_ref.filter_linear with v0 passed in → (c(L) (H, W, 3), v(L) (H, W)), linear, float64."""
    c = initial_colour(accum)
    guides = Guides(normal, position, albedo, hit, obj, sigma_normal, sigma_position, sigma_albedo, split_objects)
    v = np.asarray(v0, dtype=np.float64)
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
    return c, v


def spatial_v0(accum, normal, position, albedo, hit, obj, sigma_normal=np.inf, sigma_position=np.inf,
               sigma_albedo=np.inf, split_objects=True, **_):
    """Step 1 of rt_denoise_variance for the same parameters (the filter's other parameters are ignored)."""
    guides = Guides(normal, position, albedo, hit, obj, sigma_normal, sigma_position, sigma_albedo, split_objects)
    return variance_estimate(initial_colour(accum), guides)


def filter_moments(accum, m2, feats, **kw):
    """rt_denoise_moments as the header states it: `feats` is RayTracer.features()'s dict, m2 the moment buffer.
    → (RGBA (H, W, 4): (sqrt(c(L)), 1) where accum.w > 0, else 0; linear c(L); v0; v(L))."""
    g = (feats["normal"], feats["position"], feats["albedo"], feats["hit"], feats["object"])
    v0 = measured_v0(m2, np.asarray(accum)[..., 3], spatial_v0(accum, *g, **kw))
    lin, vl = filter_linear_given_v0(accum, v0, *g, **kw)
    out = np.zeros(lin.shape[:2] + (4,))
    has = np.asarray(accum)[..., 3] > 0
    out[has, :3] = np.sqrt(lin[has])
    out[has, 3] = 1.0
    return out, lin, v0, vl
