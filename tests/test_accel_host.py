"""CPU: the acceleration structures are host logic (built at rt_set_scene) — their invariants
are checked without a device through rt_debug_check_accel: every primitive in exactly one leaf and
inside its boxes, nested boxes, split axes and skip links, the kernels' threaded walk visiting
every leaf exactly once in all eight direction octants, smallest-face indices, normal cones."""
import numpy as np
import pytest

import cases
import scene_prep_scenes as S   # (the hand-made scenes: their prepared form is pinned by test_scene_prep_host.py)

rt = cases.rt


@pytest.mark.parametrize("name,kw", S.WORKLOADS)
def test_workload_structures(built, name, kw):
    wl = rt.workloads.get(name, **kw)
    st = rt.check_accel(wl.scene)
    n_sph = len(wl.scene.spheres)
    if n_sph:
        assert st["sphere_leaves"] >= (n_sph + 3) // 4 and st["sphere_nodes"] == 2 * st["sphere_leaves"] - 1
        assert st["sphere_depth"] <= 2 * int(np.ceil(np.log2(max(n_sph, 2)))) + 8     # SAH trees stay shallow
    big = [int(f) for f in wl.scene.meshes["face_count"] if f >= 32]
    assert st["meshes"] == len(big)
    if big:
        assert st["mesh_leaves"] >= sum((f + 1) // 2 for f in big)
        assert st["mesh_nodes"] == 2 * st["mesh_leaves"] - len(big)


def test_adversarial_spheres(built):
    st = rt.check_accel(S.adversarial_spheres())
    assert st["sphere_leaves"] > 1000


def test_degenerate_and_tiny_meshes(built):
    st = rt.check_accel(S.degenerate_meshes())
    assert st["meshes"] == 1 and st["mesh_leaves"] >= 100
    assert rt.check_accel(S.empty())["sphere_nodes"] == 0


@pytest.mark.parametrize("scale", S.PACKED_SCALES)
def test_packed_mesh_nodes_at_extreme_scales(built, scale):
    """The device's 48-byte mesh node carries half extent, sin alpha, longest edge and q as binary16
    (mesh_node_pack): rt_debug_check_accel unpacks every node and checks that each field is rounded
    to the safe side — here for meshes whose extents fall below binary16's normal range (1e-6: the
    smallest normal stands in) and above its largest value (4e4, 1e9: +inf, an unbounded box)."""
    st = rt.check_accel(S.packed_scale(scale))
    assert st["meshes"] == 1 and st["mesh_leaves"] >= 40 * 23
