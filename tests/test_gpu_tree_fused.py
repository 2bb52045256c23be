"""GPU (-m gpu): the shared decision trees are built inside pt_prefix, by the workgroup that found the glass-first
pixels (RT_OPT_PREFIX_TREE).  Whatever the trees hold, the accumulators must equal the per-sample tracing
(RT_OPT_PREFIX_TREE 0) bit for bit: workgroups whose every pixel is glass-first, nested glass, several slot ranges per
frame, an adaptive render with a block mask, and more glass-first pixels than the tree capacity."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
rt = cases.rt


def _glass_wall_scene():
    """One large dielectric sphere right in front of the camera (_glass_wall_camera): every pixel's first random event is
    glass, so every workgroup of pt_prefix builds 256 trees, and a frame holds about four times the tree capacity."""
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIELECTRIC, (1, 1, 1), 1.5)         # 0
    s.addMaterial(rt._abi.T_DIFFUSE, (0.8, 0.7, 0.6), 0.9)      # 1
    s.addMaterial(rt._abi.T_LIGHT, (1, 1, 1), 0)                # 2
    s.addMaterial(rt._abi.T_DIELECTRIC, (1, 0.9, 0.9), 2.4)     # 3
    s.addSphere((0, 0, 0), 5.9, 0)
    s.addSphere((0.5, 0.3, 1.0), 1.5, 3)                         # glass behind the glass
    s.addSphere((0, 250, 0), 120, 2)
    s.addPlane((0, -7, 0), (0, 1, 0), 1)
    return s, rt.Camera(60, 16 / 9, (0, 0, -6), 0.0, 0.0).transferData()


def _glass_stack_scene():
    """Concentric dielectric shells, touching dielectric spheres, a refractive ball and a mirror over a diffuse floor."""
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIELECTRIC, (1, 1, 1), 1.5)         # 0
    s.addMaterial(rt._abi.T_DIELECTRIC, (0.9, 1, 0.95), 1.1)    # 1
    s.addMaterial(rt._abi.T_DIELECTRIC, (1, 0.9, 0.9), 2.4)     # 2 dense: much total internal reflection
    s.addMaterial(rt._abi.T_REFRACTIVE, (1, 1, 1), 1.3)         # 3
    s.addMaterial(rt._abi.T_REFLECTIVE, (1, 1, 1), 0.9)         # 4
    s.addMaterial(rt._abi.T_DIFFUSE, (0.8, 0.8, 0.8), 0.9)      # 5
    s.addMaterial(rt._abi.T_LIGHT, (1, 1, 1), 0)                # 6
    s.addSphere((0, -250, 0), 120, 6)
    for r, m in ((2.4, 0), (1.9, 1), (1.3, 2), (0.6, 0)):       # concentric shells
        s.addSphere((0, 2.4, 4), r, m)
    s.addSphere((4.2, 3.2, 3.5), 1.8, 2)
    s.addSphere((-4.4, 3.4, 4.5), 1.6, 1)
    s.addSphere((-2.6, 4.0, 1.2), 1.0, 3)
    s.addSphere((2.3, 4.1, 0.8), 0.9, 4)
    s.addPlane((0, 5, 0), (0, 1, 0), 5)
    return s, rt.Camera(60, 16 / 9, (0, 0, -6), 0.0, 4.0).transferData()


def _frame(t, cam, first, spp, tree):
    t.setOption(t.OPT_PREFIX_TREE, tree)
    t.clear()
    t.renderSamples(cam, first, spp)
    t.sync()
    return t.readLinear().copy()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module", params=["glass_wall", "glass_stack"])
def glass(request):
    scene, cam = (_glass_wall_scene if request.param == "glass_wall" else _glass_stack_scene)()
    t = rt.RayTracer(320, 180, scene=scene, seed=cases.SEED)
    t.setArith(2)
    yield request.param, t, cam
    t.close()


@pytest.mark.parametrize("spp, first", [(1, 0), (64, 0), (200, 7)])
def test_fused_trees_change_no_bit(glass, spp, first):
    """One launch per frame: on the glass wall most glass-first pixels lie beyond the tree capacity (a quarter of the
    slots) and continue per sample, the others get full workgroups of trees."""
    name, t, cam = glass
    with_trees = _frame(t, cam, first, spp, 2)
    assert _same(with_trees, _frame(t, cam, first, spp, 0)), (name, spp)
    assert np.isfinite(with_trees).all() and with_trees[..., :3].sum() > 0


@pytest.mark.parametrize("threads", [1 << 14, 1 << 16, 100_000])
def test_fused_trees_slot_ranges(glass, threads):
    """Several slot ranges per frame (RT_OPT_MAX_THREADS_PER_LAUNCH): each range reserves its trees from zero again, and
    no range of the glass wall exceeds the capacity."""
    name, t, cam = glass
    whole = _frame(t, cam, 0, 64, 0)
    t.setOption(t.OPT_MAX_THREADS_PER_LAUNCH, threads)
    try:
        ranges = _frame(t, cam, 0, 64, 2)
    finally:
        t.setOption(t.OPT_MAX_THREADS_PER_LAUNCH, 1 << 30)
    assert _same(ranges, whole), (name, threads)


def test_fused_trees_adaptive_block_mask(glass):
    """An adaptive render: after its first rounds only the unconverged blocks' pixels run pt_prefix (the block mask)."""
    name, t, cam = glass
    out = []
    for tree in (2, 0):
        t.setOption(t.OPT_PREFIX_TREE, tree)
        st = t.renderAdaptive(cam, 2e-3, batch=32, min_spp=64, max_spp=256, block=(8, 8))
        t.sync()
        out.append((st, t.readLinear().copy(), t.sampleCounts().copy()))
    (st2, lin2, n2), (st0, lin0, n0) = out
    assert st2 == st0, name
    assert np.array_equal(n2, n0), name
    assert n2.min() < n2.max(), name     # the mask did leave blocks out
    assert _same(lin2, lin0), name
