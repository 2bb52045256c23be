"""The ray batch the degenerate scenes of tests/edge_scenes.py are queried with, shared by tests/test_edge_queries_host.py
and tests/test_gpu_edge_queries.py: what a camera makes, what a bake makes from the hit points, and what no camera makes —
directions with components that are exactly zero, the zero direction, directions far from unit length, origins on a
surface and at a sphere's centre.  Every number is finite.

    primary     the scene's 48 x 32 primary rays (policy IEEE's direction bits)
    hemisphere  one cosine-hemisphere ray per primary hit, rays.hemisphere_sets(pos, normal, 1, SEED): the origins lie ON the
                surface and the normals are as reported, so some are not unit
    special     from the eye, the first 8 sphere centres and every plane point: +-x, +-y, +-z, (1, 1, 0), (0, 1, 1), (0, 0, 0)
    scaled      all of the above again with the directions scaled by 1.1, 2 and 1e-3: out of the sphere BVH's unit-length
                gate on both sides
"""
import numpy as np

import cases
import edge_scenes as E
from test_denoise_vg_host import primary_dirs

rt = cases.rt
F32 = np.float32
SEED = 11
SCALES = (F32(1.1), F32(2.0), F32(1e-3))
DIRECTIONS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (0, 1, 1), (0, 0, 0)], F32)
SPECIAL_SPHERES = 8


def scene_hits(source, scene, rays6):
    """hitScene's (n, 12) records for (n, 6) rays from the CPU oracle (or the compiled reference: anything with
    hit(kind, scene, rays, prim)) or from a probe object of tests/chain_ref.py (hit(kind, rays))."""
    rays6 = np.ascontiguousarray(rays6, dtype=F32).reshape(-1, 6)
    if hasattr(source, "hit_triangle"):
        return source.hit(3, scene, rays6, np.zeros(len(rays6), np.uint32))
    return source.hit(3, rays6)


def primary(camera):
    """(W * H, 6): the camera's primary rays, row-major"""
    cam = np.asarray(camera, F32).reshape(12)
    d = primary_dirs(cam, E.W, E.H).reshape(-1, 3)
    return np.concatenate([np.broadcast_to(cam[:3], d.shape), d], axis=1).astype(F32)


def special(scene, camera):
    """(9 * origins, 6): DIRECTIONS from the eye, the first SPECIAL_SPHERES sphere centres and every plane point"""
    eye = np.asarray(camera, F32).reshape(12)[None, :3]
    origins = np.concatenate([eye, scene.spheres["pos"][:SPECIAL_SPHERES, :3], scene.planes["pos"][:, :3]]).astype(F32)
    return np.concatenate([np.repeat(origins, len(DIRECTIONS), axis=0), np.tile(DIRECTIONS, (len(origins), 1))], axis=1)


def edge_rays(source, scene, camera):
    """The batch for (scene, camera) → (n, 6) float32, n = 4 (W H + hits + special); `source` as scene_hits takes it."""
    prim = primary(camera)
    out = scene_hits(source, scene, prim)
    hit = out[:, 0] > 0
    pos, normal = out[hit, 2:5], out[hit, 5:8]
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((normal.astype(np.float64) ** 2).sum(1))
    ok = np.isfinite(length) & (length > 0) & np.isfinite(pos).all(1)      # (a hit without a normal has no hemisphere)
    hemi = rt.rays.hemisphere_sets(pos[ok], normal[ok], 1, SEED).reshape(-1)
    base = np.concatenate([prim, np.concatenate([hemi["o"], hemi["d"]], axis=1), special(scene, camera)]).astype(F32)
    parts = [base]
    for scale in SCALES:
        c = base.copy()
        c[:, 3:] = (base[:, 3:] * scale).astype(F32)
        parts.append(c)
    rays6 = np.concatenate(parts)
    assert np.isfinite(rays6).all()
    return rays6


def special_index(scene, camera, n):
    """The positions of the special rays, directions as given (the unscaled copy), in edge_rays' batch of n rays"""
    m = len(special(scene, camera))
    assert n % (1 + len(SCALES)) == 0
    base = n // (1 + len(SCALES))
    return np.arange(base - m, base)
