"""Float64 reference of the textured path, written from the definition in DESIGN.md §3 and from the scene arrays alone:
primary rays of the camera block, Möller–Trumbore against every face, barycentric uv, and the bilinear edge-clamp texel.
Nothing here calls or restates the float32 copies (texture_rgb in pt_device.hpp / pt_oracle.c, the read_imagef stand-in
of ref_shim.cpp, chain_ref.texel); it is what tests/test_texture_sampler_host.py and tests/test_gpu_texture_sampler.py
compare those with.

The sampler, per axis (W texels, normalized coordinate s):
    U  = s * W - 0.5, clamped to [-1, W]; NaN counts as -1
    i0 = floor(U), a = U - i0, i1 = i0 + 1, both indices clamped to [0, W - 1]
    T  = (1-a)(1-b) T[j0,i0] + a(1-b) T[j0,i1] + (1-a) b T[j1,i0] + a b T[j1,i1]
so that outside the image the colour is the constant edge texel."""
import numpy as np

F64 = np.float64
EDGE_MARGIN = 1e-3        # world units: pixels whose ray meets a face's plane this close to one of its edges are left out


def _axis(s, n):
    s = np.asarray(s, F64)
    with np.errstate(invalid="ignore", over="ignore"):
        U = s * n - 0.5
        U = np.where(np.isnan(U), -1.0, np.minimum(np.maximum(U, -1.0), float(n)))
    i0 = np.floor(U)
    a = U - i0
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), a


def texel64(textures, s, t, layer):
    """The definition in float64 → (n, 3).  `layer` as the kernels select it: texture_ID < layers ? texture_ID : 0."""
    T = np.asarray(textures, F64)
    layers, H, W = T.shape[:3]
    layer = np.asarray(layer, np.int64)
    layer = np.where(layer < layers, layer, 0)
    i0, i1, a = _axis(s, W)
    j0, j1, b = _axis(t, H)
    a, b = a[:, None], b[:, None]
    return ((1 - a) * (1 - b) * T[layer, j0, i0, :3] + a * (1 - b) * T[layer, j0, i1, :3]
            + (1 - a) * b * T[layer, j1, i0, :3] + a * b * T[layer, j1, i1, :3])


def unclamped_coordinates(textures, s, t):
    """(s W - 0.5, t H - 0.5) in float64: the texel coordinates before the clamp."""
    _, H, W = np.asarray(textures).shape[:3]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(s, F64) * W - 0.5, np.asarray(t, F64) * H - 0.5


def primary_rays(cam, w, h):
    """(origin (3,), unit directions (h, w, 3)) of the 12-float camera block, in float64: pixel (x, y) looks through
    lower_left_corner + (x / w) horizontal + (y / h) vertical."""
    cam = np.asarray(cam, F64)
    ys, xs = np.mgrid[0:h, 0:w]
    d = cam[3:6] + (xs / w)[..., None] * cam[6:9] + (ys / h)[..., None] * cam[9:12]
    return cam[0:3].copy(), d / np.linalg.norm(d, axis=2, keepdims=True)


def _segment_distance(p, a, b):
    ab = b - a
    L2 = float(ab @ ab)
    if L2 == 0.0:
        return np.linalg.norm(p - a, axis=-1)
    k = np.clip(((p - a) @ ab) / L2, 0.0, 1.0)
    return np.linalg.norm(p - (a + k[..., None] * ab), axis=-1)


def first_hits(scene, cam, w, h):
    """The nearest front-facing mesh face every primary ray meets → dict of (h, w) arrays: hit, u, v (texture
    coordinates), tex (the mesh's texture_ID), t, and `edge`, the smallest distance in world units between a face's edge
    and the point where the ray meets that face's plane (over all faces: pixels with edge < EDGE_MARGIN may hit or miss
    differently in float32 and are left out by the callers).  Faces seen from behind are ignored, as the kernels do."""
    o, d = primary_rays(cam, w, h)
    V = np.asarray(scene.vertices, F64)[:, :3]
    UV = np.asarray(scene.texture_uv, F64)
    out = dict(hit=np.zeros((h, w), bool), u=np.zeros((h, w)), v=np.zeros((h, w)), tex=np.zeros((h, w), np.int64),
               t=np.full((h, w), np.inf), edge=np.full((h, w), np.inf))
    for m in scene.meshes:
        va, ia = int(m["vertex_anchor"]), int(m["index_anchor"])
        for f in range(int(m["face_count"])):
            ids = va + np.asarray(scene.indices[ia + 3 * f: ia + 3 * f + 3], np.int64)
            A, B, C = V[ids]
            n = np.cross(B - A, C - A)
            if not n.any():
                continue
            den = d @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((A - o) @ n) / den
            p = o + t[..., None] * d
            ahead = np.isfinite(t) & (t > 0)
            e = np.minimum(np.minimum(_segment_distance(p, A, B), _segment_distance(p, B, C)), _segment_distance(p, C, A))
            out["edge"] = np.where(ahead, np.minimum(out["edge"], e), out["edge"])
            # barycentrics of p in the face: p = A + bu (B - A) + bv (C - A)
            nn = float(n @ n)
            bu = np.cross(p - A, C - A) @ n / nn
            bv = np.cross(B - A, p - A) @ n / nn
            inside = ahead & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (den < 0) & (t < out["t"])
            wa = 1.0 - bu - bv
            with np.errstate(over="ignore", invalid="ignore"):
                u = UV[ids[0], 0] * wa + UV[ids[1], 0] * bu + UV[ids[2], 0] * bv
                v = UV[ids[0], 1] * wa + UV[ids[1], 1] * bu + UV[ids[2], 1] * bv
            for k, val in (("u", u), ("v", v), ("t", t)):
                out[k] = np.where(inside, val, out[k])
            out["tex"] = np.where(inside, int(m["texture_ID"]), out["tex"])
            out["hit"] |= inside
    return out


def contrast_slope(textures):
    """Largest adjacent-texel contrast x texels per unit uv, summed over both axes: how fast the bilinear colour can change
    per unit of uv."""
    T = np.asarray(textures, F64)[..., :3]
    _, H, W = T.shape[:3]
    cx = np.abs(np.diff(T, axis=2)).max() if W > 1 else 0.0
    cy = np.abs(np.diff(T, axis=1)).max() if H > 1 else 0.0
    return cx * W + cy * H


def tolerance(textures, uv_max, c):
    """c * 2^-24 * L with L = contrast_slope * max(1, |uv|max) + 4 (4 ulp of a texel below 1, in units of 2^-24)."""
    return c * 2.0 ** -24 * (contrast_slope(textures) * max(1.0, float(uv_max)) + 4.0)
