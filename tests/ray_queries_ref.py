"""The reference side of the ray queries (rt_intersect_rays, rt_occluded_rays), shared by tests/test_ray_queries_host.py and
tests/test_gpu_ray_queries.py: occlusion as its definition over the CPU oracle's hitScene — a record is occluded iff the
first hit's t is below its bound in binary32 — the face-order scene, and the bounds the GPU test cycles through."""
import numpy as np

import cases

rt = cases.rt
A = rt._abi
F32 = np.float32
MIN_DISTANCE, MAX_DISTANCE = F32(0.001), F32(1000.0)


def first_hit_t(oracle, scene, rays6):
    """t of hitScene (oracle.hit kind 3) for (n, 6) rays (origin, direction), +inf on a miss → (n,) float32"""
    rays6 = np.ascontiguousarray(rays6, dtype=F32).reshape(-1, 6)
    out = oracle.hit(3, scene, rays6, np.zeros(len(rays6), np.uint32))
    return np.where(out[:, 0] != 0, out[:, 1], F32(np.inf)).astype(F32)


def occluded(t, bounds):
    """The definition: t < bound in binary32 (false for a NaN bound) → (n,) bool"""
    t, bounds = np.asarray(t, F32), np.broadcast_to(np.asarray(bounds, F32), np.shape(t))
    with np.errstate(invalid="ignore"):
        return t < bounds


def occluded_ref(oracle, scene, rays6, bounds):
    return occluded(first_hit_t(oracle, scene, rays6), bounds)


def cycled_bounds(t):
    """Per-record bounds around each record's own first-hit t (+inf on a miss), record k taking case k mod 12:
    t, the float above it, the float below it, t / 2, 2 t, +inf, NaN, 0, -1, MIN_DISTANCE, 1000, the float above 1000."""
    t = np.asarray(t, F32)
    inf = F32(np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = [t, np.nextafter(t, inf), np.nextafter(t, -inf), t / F32(2), t * F32(2), np.full_like(t, inf),
                np.full_like(t, np.nan), np.zeros_like(t), np.full_like(t, -1), np.full_like(t, MIN_DISTANCE),
                np.full_like(t, MAX_DISTANCE), np.full_like(t, np.nextafter(MAX_DISTANCE, inf))]
    rows = np.stack(rows).astype(F32)
    return rows[np.arange(len(t)) % len(rows), np.arange(len(t))]


FACE_ORDER_FACES = 36


def face_order_scene():
    """One model of one 36-face mesh in front of the ray (0, 0, 0) → (0, 0, 1): face 0 is the triangle (-1, -1, 6), (0, 1, 6),
    (1, -1, 6), face 1 the same at z = 3, the other 34 the same shape at x = 50 + 3 k, z = 5 — enough faces for a mesh BVH.
    The mesh reports its FIRST front-facing face in face order: t = 6, the far one (and t = 5 from (50, 0, 0))."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_DIFFUSE, (0.8, 0.8, 0.8), 1)
    tri = np.array([(-1, -1, 0), (0, 1, 0), (1, -1, 0)], F32)
    shifts = [(0, 0, 6), (0, 0, 3)] + [(50 + 3 * k, 0, 5) for k in range(FACE_ORDER_FACES - 2)]
    verts = np.concatenate([tri + np.array(sh, F32) for sh in shifts])
    s.addMesh(verts, None, np.arange(len(verts), dtype=np.uint32))
    s.addModel(1, 0)
    return s


FACE_ORDER_RAY = np.array([0, 0, 0, 0, 0, 1], F32)
# (bound, occluded): the far face at t = 6 is the mesh's report, the nearer face at z = 3 is not
FACE_ORDER_CASES = [(4.0, False), (6.5, True), (6.0, False)]


def box_rays(scene, n, stream):
    """n arbitrary rays for `scene`: origins uniform in the box of its sphere centres, plane points and vertices, grown by
    a fifth, directions uniform on the sphere (unit length to float32 rounding) → (n, 6) float32"""
    pts = [scene.spheres["pos"][:, :3], scene.planes["pos"][:, :3], scene.vertices[:, :3]]
    pts = np.concatenate([p.reshape(-1, 3) for p in pts if len(p)]).astype(np.float64)
    lo, hi = pts.min(0), pts.max(0)
    lo, hi = np.maximum(lo, -60.0), np.minimum(hi, 60.0)   # (a plane's point may lie far out)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2 * 1.2, 1.0)
    u = rt.workloads.uniforms(n, stream, cases.SEED).astype(np.float64)
    u2 = rt.workloads.uniforms(n, stream + 1, cases.SEED).astype(np.float64)
    o = mid + (2 * u[:, :3] - 1) * half
    z, phi = 2 * u2[:, 0] - 1, 2 * np.pi * u2[:, 1]
    r = np.sqrt(np.maximum(0.0, 1 - z * z))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    return np.concatenate([o, d], axis=1).astype(F32)
