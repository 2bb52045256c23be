"""Scenes that show the texel fetch and nothing else, shared by tests/test_texture_sampler_host.py and
tests/test_gpu_texture_sampler.py.

The eye sits at the origin inside a white light sphere of radius 50 and looks at one textured quad.  A sample that hits the
quad scatters once (extra_data 1, colours mix by min) and always reaches the light, so its radiance IS the texel, bit for
bit; a sample that misses the quad sees the light, (1, 1, 1).  The quad is cut into one horizontal band per texture layer,
each band a mesh of two faces with its own texture_ID; uv is one affine function over the whole quad, from `uv0` at the
first corner to `uv1` at the opposite one.  Texture widths and heights differ, so that a row stride or a u / v swap
shows."""
import numpy as np

import cases

rt = cases.rt
A = rt._abi
F32 = np.float32
W, H = 64, 40

# texture name → (height, width, layers)
TEXTURES = {"1x1": (1, 1, 2), "5x3": (5, 3, 3), "2x7": (2, 7, 1), "33x17": (33, 17, 2), "64x64": (64, 64, 1)}
# uv window name → (uv at corner (-3, -2), uv at corner (3, 2))
WINDOWS = {
    "inside": ((0.07, 0.11), (0.93, 0.86)),
    "straddle": ((-0.6, -0.4), (1.7, 1.5)),
    "far": ((-40.0, -40.0), (40.0, 40.0)),
    "exact01": ((0.0, 0.0), (1.0, 1.0)),
    "huge": ((-1e30, 1e30), (1e30, -1e30)),
}
# the quad's corners in the order (-,-), (+,-), (+,+), (-,+): facing the eye at z = 5, and seen at a slant
QUADS = {
    "facing": ((-3, -2, 5), (3, -2, 5), (3, 2, 5), (-3, 2, 5)),
    "slant": ((-3, -2, 3.2), (3, -2, 6.2), (3, 2, 7.8), (-3, 2, 4.8)),
}
# (texture, window, quad): every texture and every window at least once, the small odd texture through all windows
CASES = [
    ("1x1", "straddle", "facing"),
    ("5x3", "inside", "facing"), ("5x3", "straddle", "facing"), ("5x3", "far", "facing"), ("5x3", "exact01", "facing"),
    ("5x3", "huge", "facing"), ("5x3", "straddle", "slant"),
    ("2x7", "straddle", "facing"), ("2x7", "far", "facing"),
    ("33x17", "inside", "facing"), ("33x17", "straddle", "facing"), ("33x17", "exact01", "facing"), ("33x17", "inside", "slant"),
    ("64x64", "straddle", "facing"), ("64x64", "huge", "facing"),
]


def case_id(case):
    return "-".join(case)


def random_texture(name):
    h, w, layers = TEXTURES[name]
    rng = np.random.RandomState(1000 + 64 * h + w)
    t = np.ones((layers, h, w, 4), F32)
    t[..., :3] = (0.05 + 0.9 * rng.random_sample((layers, h, w, 3))).astype(F32)
    return t


def build(texture, window, quad):
    """→ (scene, camera block, largest |uv| at a vertex)."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_TEXTURED, (1, 1, 1), 1)   # 0
    s.addMaterial(A.T_LIGHT, (1, 1, 1), 0)      # 1
    s.addSphere((0, 0, 0), 50, 1)
    tex = random_texture(texture)
    layers = tex.shape[0]
    c = np.asarray(QUADS[quad], np.float64)
    (u0, v0), (u1, v1) = WINDOWS[window]

    def corner(a, b):
        """Position and uv at quad coordinates (a, b) in [0, 1]^2 (the four corners are coplanar)."""
        p = c[0] + a * (c[1] - c[0]) + b * (c[3] - c[0])
        return p, (u0 + a * (u1 - u0), v0 + b * (v1 - v0))

    uv_max = 0.0
    for k in range(layers):
        b0, b1 = k / layers, (k + 1) / layers
        pts = [corner(0, b0), corner(1, b0), corner(1, b1), corner(0, b1)]
        pos = np.array([p for p, _ in pts], F32)
        uv = np.array([q for _, q in pts], F32)
        idx = [0, 2, 1, 0, 3, 2]
        n = np.cross(pos[2].astype(np.float64) - pos[0], pos[1].astype(np.float64) - pos[0])
        if n @ pos[0] > 0:      # the faces must look at the eye (the origin): a face seen from behind is no hit
            idx = [0, 1, 2, 0, 2, 3]
        s.addMesh(pos, uv, idx, k)
        uv_max = max(uv_max, float(np.abs(uv).max()))
    s.addModel(layers, 0)
    s.setTextures(tex)
    cam = rt.Camera(60, F32(W) / F32(H), (0.0, 0.0, 0.0), 0.0, 0.0).transferData()
    return s, cam, uv_max
