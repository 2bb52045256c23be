"""GPU (-m gpu): the sample queue reads its staged scene tables from LDS wherever they are staged (csrc/pt_queue.hpp
PT_TABLES_BY_COUNT: presence asked of the scene's counts — the pointer calls a table at LDS address 0 absent) and changes no bit.

Frames of the fused path against the direct path pt_render — which this does not touch — with == as uint32: C2, C3, the
all-kinds scene and the nested-glass stack; 61 x 37 and 7 x 5; policies `ieee` and `rocm-opencl`; counts 1, 3, 64, 65, 200;
wave fill off and on; seven spheres whose radii span 2^-20 ... 2^20 on a plane (winner records at the ends of the range:
the sphere normal divides by the staged radius); more spheres than the LDS winner table holds and more materials than the
material table holds, both without the sphere BVH (the global-memory arm of each presence test IN the changed kernel — every
fused launch here is checked to have taken it, through the launch plan); rank 1 of 3 of a sharded context; two calls of 64 on
one accumulator; and, after rt_set_scene with other radii and after a policy change, frames equal to a fresh context's
(the staged glass constants are the policy's divisions)."""
import numpy as np
import pytest

import cases
import edge_scenes

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
F32 = np.float32

COUNTS = (1, 3, 64, 65, 200)
SIZES = {"ragged": (61, 37), "tiny": (7, 5)}
ARITHS = ("ieee", "rocm-opencl")
RADII = (1e-3, 0.37, 1.0, 3.0, 1000.0, 2.0 ** -20, 2.0 ** 20)
_SCENES = {}


def _camera(w, h, pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0):
    return rt.Camera(60, F32(w) / F32(h), pos, yaw, pitch).transferData()


def _primary_dir(cam, s, t):
    """Direction of the primary ray at frame coordinates (s, t), in float64 (where to PUT a sphere, not what to expect)."""
    cam = np.asarray(cam, dtype=np.float64)
    d = cam[3:6] + s * cam[6:9] + t * cam[9:12]
    return d / np.linalg.norm(d)


def _radii_scene(w, h, probe=False, scale=1.0):
    """Seven spheres of the radii RADII (times `scale`) over a floor, each where primary rays reach it within the reference's
    in_range [1e-3, 1000]: the small ones centred ON the primary ray of a pixel, a few radii from the eye; the huge ones
    to the left and to the right of the view, their surfaces behind the others.  probe: every sphere is a light of its own colour (which spheres
    does some pixel see first?); otherwise they are diffuse, glass and mirror, and the floor is the light."""
    s = rt.SceneCreator()
    cam = _camera(w, h)
    if probe:
        for k in range(len(RADII)):
            s.addMaterial(A.T_LIGHT, ((k + 1) / 8.0, 0.0, 0.0), 0)
        s.addMaterial(A.T_DIFFUSE, (0.0, 0.5, 0.0), 1)
        mats, floor = list(range(len(RADII))), len(RADII)
    else:
        s.addMaterial(A.T_DIFFUSE, (0.8, 0.7, 0.6), 1)
        s.addMaterial(A.T_DIELECTRIC, (1, 1, 1), 1.5)
        s.addMaterial(A.T_REFLECTIVE, (0.9, 0.9, 0.9), 1)
        s.addMaterial(A.T_LIGHT, (1, 1, 1), 0)
        mats, floor = [0, 1, 2, 0, 0, 0, 2], 3
    eye = np.asarray(cam, dtype=np.float64)[0:3]
    # (frame coordinates of pixel centres that exist in both frame sizes: s = x / w, t = y / h with x = y = 0 ... )
    spots = {0: (0.0, 0.0), 5: (0.0, 3.0 / 5.0 if h == 5 else 22.0 / 37.0)}
    for k, r in enumerate(RADII):
        r = r * scale
        if k in spots:        # 1e-3 and 2^-20: on a pixel's own ray, the near surface beyond RT_MIN_DISTANCE
            d = _primary_dir(cam, *spots[k])
            c = eye + d * (max(4.0 * r, 2e-3) + r)
        elif k == 1:
            c = eye + _primary_dir(cam, 0.3, 0.45) * 3.0
        elif k == 2:
            c = eye + _primary_dir(cam, 0.7, 0.45) * 5.0
        elif k == 3:
            c = eye + _primary_dir(cam, 0.5, 0.75) * 12.0
        elif k == 4:          # r = 1000: to the left, its surface 15 units from the eye — it fills the frame's left part
            c = eye + np.array([-1.0, 0.0, 0.1]) / np.sqrt(1.01) * (15.0 + r)
        else:                 # r = 2^20: to the right and a little behind, 200 units away — nearly a wall across the right part
            c = eye + np.array([1.0, 0.0, -0.2]) / np.sqrt(1.04) * (200.0 + r)
        s.addSphere(tuple(float(v) for v in c), r, mats[k])
    s.addPlane((0, 6, 0), (0, 1, 0), floor)
    return s, cam


def _workload(case, size):
    if (case, size) not in _SCENES:
        w, h = SIZES[size]
        if case == "nested_glass":
            scene, _ = edge_scenes.get("nested_spheres")
            cam = _camera(w, h)
        elif case == "radii":
            scene, cam = _radii_scene(w, h)
        elif case == "many_spheres":     # more spheres than PT_LDS_WINNERS: hit_finish reads the global sphere records
            wl = rt.workloads.get("c2", width=w, height=h)
            u = rt.workloads.uniforms(A.LDS_WINNERS, 5, cases.SEED)
            for k in range(A.LDS_WINNERS):
                wl.scene.addSphere((float(u[k, 0] * 8 - 4), float(u[k, 1] * 4 - 2), float(6 + u[k, 2] * 4)), 0.15 + 0.2 * float(u[k, 3]), k % 4)
            scene, cam = wl.scene, wl.camera
            assert len(scene.spheres) > A.LDS_WINNERS
        elif case == "many_materials":   # more materials than PT_LDS_MATERIALS: load_material and glass_terms read global memory
            wl = rt.workloads.get("c2", width=w, height=h)
            for k in range(A.LDS_MATERIALS):
                wl.scene.addMaterial(A.T_DIFFUSE, (0.1 + 0.01 * k, 0.5, 0.9), 1.0)
            scene, cam = wl.scene, wl.camera
            assert len(scene.materials) > A.LDS_MATERIALS
        else:
            wl = rt.workloads.get(case, width=w, height=h, **({"tex_size": 8} if case == "c3" else {}))
            scene, cam = wl.scene, wl.camera
        _SCENES[case, size] = (scene, cam, w, h)
    return _SCENES[case, size]


def _frame(t, cam, first, count, fused, calls=1):
    t.setOption(t.OPT_PREFIX_SHARING, 1 if fused else 0)
    t.setOption(t.OPT_SAMPLE_QUEUE, 1 if fused else 0)
    t.clear()
    for k in range(calls):
        t.renderSamples(cam, first + k * count, count)
    t.sync()
    return t.readLinear().copy()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _ran_the_changed_kernel(t):
    """The last fused launch took pt_samples_q<COUNT = false, ACCEL = false, ...>: the instantiations that ask by count."""
    facts, plan = t.lastSamplePlan()
    return plan["family"] == A.PLAN_QUEUE and plan["accel"] == 0 and facts["count_enabled"] == 0


def _compare(t, cam, key, counts=COUNTS, fills=(0, 1)):
    for count in counts:
        direct = _frame(t, cam, 0, count, False)
        for fill in fills:
            t.setOption(t.OPT_WAVE_FILL, fill)
            assert _same(_frame(t, cam, 0, count, True), direct), key + (count, fill)
            assert _ran_the_changed_kernel(t), key + (count, fill, t.lastSamplePlan())


def _fresh(scene, cam, w, h, arith, count=64):
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        return _frame(t, cam, 0, count, True)
    finally:
        t.close()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("size", ["ragged", "tiny"])
@pytest.mark.parametrize("case", ["c2", "c3", "all_kinds", "nested_glass", "radii"])
def test_fused_frames_equal_the_direct_path(case, size, arith):
    scene, cam, w, h = _workload(case, size)
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        _compare(t, cam, (case, size, arith))
    finally:
        t.close()


@pytest.mark.parametrize("size", ["ragged", "tiny"])
def test_the_radii_scene_shows_its_spheres(size):
    """On the CPU oracle: at least five of the seven spheres are the first hit of some pixel (the reference's in_range keeps
    t within [1e-3, 1000]; the same geometry with every sphere a light of its own colour)."""
    import oracle
    w, h = SIZES[size]
    scene, cam = _radii_scene(w, h, probe=True)
    orc = oracle.Oracle()
    img, _ = orc.render(scene, cam, orc.make_random_table(cases.SEED), w, h, 0)
    red = np.square(img[..., 0].astype(np.float64))   # (the image is in gamma space: sqrt of the light's colour)
    seen = {k for k in range(len(RADII)) if (np.abs(red - (k + 1) / 8.0) < 1e-3).any()}
    assert len(seen) >= 5, sorted(seen)
    assert {1, 2, 3, 4} <= seen, sorted(seen)     # (the ordinary ones and r = 1000 at the least)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", ["many_spheres", "many_materials"])
def test_a_table_over_its_cap_is_read_from_global_memory(case, arith):
    scene, cam, w, h = _workload(case, "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    # 64 spheres and more get the sphere BVH by default, and with it pt_samples_q<..., ACCEL = true>, which keeps the pointer
    # test: without the BVH the changed kernel scans all of them and rebuilds the winner from the global records
    t.setOption(t.OPT_ACCEL, 0)
    try:
        _compare(t, cam, (case, arith), counts=(3, 64, 65))
        facts, _ = t.lastSamplePlan()
        if case == "many_spheres":
            assert facts["sphere_count"] > A.LDS_WINNERS and facts["sphere_bvh"] == 0, facts
        else:
            assert facts["material_count"] > A.LDS_MATERIALS, facts
    finally:
        t.close()


@pytest.mark.parametrize("arith", ARITHS)
def test_sharded_context_rank_1_of_3(arith):
    scene, cam, w, h = _workload("c2", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    t.setShard(1, 3)
    try:
        _compare(t, cam, ("c2", "rank 1 of 3", arith), counts=(3, 64, 65))
    finally:
        t.close()


@pytest.mark.parametrize("arith", ARITHS)
def test_two_calls_of_64_on_one_accumulator(arith):
    scene, cam, w, h = _workload("radii", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        assert _same(_frame(t, cam, 0, 64, True, calls=2), _frame(t, cam, 0, 64, False, calls=2))
    finally:
        t.close()


def test_other_radii_and_another_policy_leave_nothing_stale():
    """rt_set_scene with every radius halved, then rocm-opencl -> ieee -> rocm-opencl: each frame equals a fresh context's."""
    w, h = SIZES["ragged"]
    scene_a, cam = _radii_scene(w, h)
    scene_b, _ = _radii_scene(w, h, scale=0.5)
    t = rt.RayTracer(w, h, scene=scene_a, seed=cases.SEED)
    t.setArith("rocm-opencl")
    try:
        a = _frame(t, cam, 0, 64, True)
        assert _same(a, _fresh(scene_a, cam, w, h, "rocm-opencl"))
        t.setScene(scene_b)
        b = _frame(t, cam, 0, 64, True)
        assert _same(b, _fresh(scene_b, cam, w, h, "rocm-opencl"))
        assert not _same(a, b)
        for arith in ("ieee", "rocm-opencl"):
            t.setArith(arith)
            got = _frame(t, cam, 0, 64, True)
            assert _same(got, _fresh(scene_b, cam, w, h, arith)), arith
            assert _same(got, _frame(t, cam, 0, 64, False)), arith
        t.setScene(scene_a)
        assert _same(_frame(t, cam, 0, 64, True), a)
    finally:
        t.close()
