"""The scenes whose prepared form (what rt_set_scene uploads) is pinned by tests/golden/scene_prep.json: every
parametrisation of tests/test_accel_host.py (which takes its hand-made scenes from here), every scene of
tests/edge_scenes.py, a scene with a NaN sphere centre and one with meshes of 31 and 32 faces (the mesh-BVH threshold).

SCENES: name → builder() → SceneCreator."""
import numpy as np

import cases
import edge_scenes as E

rt = cases.rt
F32 = np.float32

WORKLOADS = [("c2", {}), ("c4", dict(n_spheres=100000)), ("c4", dict(n_spheres=777)), ("c5", {}),
             ("c5", dict(segments=24, rings=16)), ("c3", dict(tex_size=8)), ("all_kinds", {})]
PACKED_SCALES = [1e-6, 3e-3, 1.0, 4e4, 1e9]


def workload_key(name, kw):
    return "workload/" + "_".join([name] + ["%s=%s" % kv for kv in sorted(kw.items())])


def adversarial_spheres():
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
    u = rt.workloads.uniforms(5000, 9)
    pos = np.stack([u[:, 0] * 40 - 20, u[:, 1] * 8 - 4, u[:, 2] * 40 - 10], 1).astype(np.float32)
    s.addSpheres(pos, (0.02 + 0.6 * u[:, 3] ** 3).astype(np.float32), np.zeros(5000, np.uint32))
    s.addSpheres(pos[:300], np.full(300, 0.25, np.float32), np.zeros(300, np.uint32))      # coincident centres
    s.addSpheres(np.zeros((40, 3), np.float32), np.linspace(0.1, 4, 40).astype(np.float32), np.zeros(40, np.uint32))
    s.addSphere((0, -5000, 0), 4000, 0)
    s.addSphere((1e5, 0, 1e5), 1e-5, 0)
    s.addSphere((3, 3, 3), -1.5, 0)                                                        # negative radius
    return s


def degenerate_meshes():
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
    pos, uv, idx = rt.workloads.uv_sphere(16, 10)
    pos = pos.copy()
    pos[3:6] = pos[3]                       # a zero-area face
    pos[30:33, :] = pos[30:33, :] * np.float32(1e-20)   # a microscopic face at the origin
    s.addMesh(pos, uv, idx)
    s.addMesh(pos[:9] + np.float32(5), uv[:9], idx[:9])   # 3 faces: below the BVH threshold
    s.addModel(2, 0)
    return s


def empty():
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
    return s


def packed_scale(scale):
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIELECTRIC, (1, 1, 1), 1.3)
    pos, uv, idx = rt.workloads.uv_sphere(40, 24, radius=2.0 * scale, centre=(3.0 * scale, -1.0 * scale, 2.0 * scale))
    s.addMesh(pos, uv, idx)
    s.addModel(1, 0)
    return s


def nan_sphere():
    """72 ordinary spheres (above the sphere-BVH threshold) and one whose centre has a NaN: rt_set_scene builds no
    sphere tree, the brute-force loop handles the sphere as the reference does."""
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
    u = rt.workloads.uniforms(72, 5)
    pos = np.stack([u[:, 0] * 16 - 8, u[:, 1] * 10 - 5, 7 + u[:, 2] * 10], 1).astype(F32)
    s.addSpheres(pos, (F32(0.25) + F32(0.5) * u[:, 3]).astype(F32), np.zeros(72, np.uint32))
    s.addSphere((1.0, float("nan"), 9.0), 1.0, 0)
    return s


def threshold_31_32():
    """One model of two meshes, 31 faces (face scan) and 32 faces (the smallest mesh with a BVH): no walk jobs."""
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
    pos, uv, idx = rt.workloads.uv_sphere(16, 10)
    for n in (31, 32):
        s.addMesh(pos[:3 * n] + np.float32(n), uv[:3 * n], idx[:3 * n])
    s.addModel(2, 0)
    return s


SCENES = {}
for _name, _kw in WORKLOADS:
    SCENES[workload_key(_name, _kw)] = (lambda n=_name, k=_kw: rt.workloads.get(n, **k).scene)
SCENES.update(adversarial_spheres=adversarial_spheres, degenerate_meshes=degenerate_meshes, empty=empty,
              nan_sphere=nan_sphere, threshold_31_32=threshold_31_32)
for _s in PACKED_SCALES:
    SCENES["packed_scale/%g" % _s] = (lambda sc=_s: packed_scale(sc))
for _e in sorted(E.SCENES):
    SCENES["edge/" + _e] = (lambda e=_e: E.get(e)[0])
