"""GPU (-m gpu): the sample queue's mesh-free kernels gather only the random-table entries an interaction reads
(csrc/pt_queue.hpp PT_RND_BY_USE, pt_device.hpp fetch_rnd_by_use: randomVec's entry at a diffuse or textured vertex, random's
at a dielectric one, nothing at a mirror or a refractive one) and change no bit.

Frames of the fused path against the direct path pt_render — which this does not touch — with == as uint32, at 61 x 37 and
below, under policies `ieee` and `rocm-opencl`: C2, spheres of every material kind (a textured one among them), the nested
glass shells, a scene whose only material besides the light is dielectric (every lane reads random, none randomVec) and one
of mirrors and a light (no gather at all) — these run the changed kernels, GEOM 0 — and C3 and the all-kinds scene, whose
meshes take GEOM 1: its kernels keep both gathers (fetch_rnd_b, now put together from the two reads); counts 1, 8, 23 (no trees: dielectric vertices in plain records), 24, 64 (the COUNT_LOG2 = 6 instantiation),
65, 200; trees off and on, wave fill off and on — every fused launch is checked, through the launch plan, to have run
pt_samples_q<COUNT = false, ACCEL = false, ...>; two calls of 64 on one accumulator (first_sample != 0); renderAgain batches
served from look-ahead frames (queue_replay reads the slots); a frame with one live pixel and an all-sky frame; rank 1 of 3
of a sharded context."""
import numpy as np
import pytest

import cases
import edge_scenes
from test_gpu_lookahead import Pair

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
F32 = np.float32

W, H = 61, 37
COUNTS = (1, 8, 23, 24, 64, 65, 200)
ARITHS = ("ieee", "rocm-opencl")
SCENES = ("c2", "c3", "all_kinds", "kinds_spheres", "nested_glass", "glass_only", "mirrors_only")
MESHES = ("c3", "all_kinds")   # GEOM 1
_SCENES = {}


def _camera(w, h):
    return rt.Camera(60, F32(w) / F32(h), (0.0, 0.0, 0.0), 0.0, 0.0).transferData()


def _glass_only():
    """Dielectric spheres, one inside the other's view, in front of a dielectric floor, all inside a light: the only
    interactions are t_dielectric ones."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_DIELECTRIC, (1, 1, 1), 1.5)
    s.addMaterial(A.T_DIELECTRIC, (0.9, 0.8, 0.7), 1.3)
    s.addMaterial(A.T_LIGHT, (1, 1, 1), 0)
    s.addSphere((0, 0, 0), 60, 2)
    s.addSphere((-1.5, 0.5, 7), 2, 0)
    s.addSphere((2, -0.5, 6), 1.5, 1)
    s.addSphere((0.5, 0, 12), 3, 1)
    s.addPlane((0, 4, 0), (0, 1, 0), 0)
    return s


def _mirrors_only():
    """Mirrors that lose a little at each bounce and a light: no interaction reads the table."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_REFLECTIVE, (0.9, 0.9, 0.9), 0.95)
    s.addMaterial(A.T_REFLECTIVE, (0.9, 0.6, 0.4), 0.9)
    s.addMaterial(A.T_LIGHT, (1, 1, 1), 0)
    s.addSphere((0, -30, 10), 20, 2)
    s.addSphere((-2, 0.5, 7), 2, 0)
    s.addSphere((2, 0, 6), 1.5, 1)
    s.addPlane((0, 4, 0), (0, 1, 0), 0)
    return s


def _kinds_spheres():
    """A sphere of every material kind over a diffuse floor, under a light: an interaction of every kind in the mesh-free
    kernel, the textured one with a texture of 4 x 4 texels (a sphere's hit has u = v = 0: one texel)."""
    s = rt.SceneCreator()
    for kind, colour, extra in ((A.T_DIFFUSE, (0.8, 0.7, 0.6), 1), (A.T_REFLECTIVE, (0.9, 0.9, 0.9), 0.9),
                                (A.T_DIELECTRIC, (1, 1, 1), 1.5), (A.T_REFRACTIVE, (0.9, 1, 0.9), 1.3),
                                (A.T_TEXTURED, (1, 1, 1), 1), (A.T_LIGHT, (1, 1, 1), 0)):
        s.addMaterial(kind, colour, extra)
    u = rt.workloads.uniforms(16, 3, cases.SEED)
    s.setTextures((0.2 + 0.7 * u[:, :4]).reshape(1, 4, 4, 4))
    s.addSphere((0, -40, 8), 30, 5)
    for k, x in enumerate((-5.0, -2.5, 0.0, 2.5, 5.0)):
        s.addSphere((x, 1.5 - 0.4 * k, 9 + 0.5 * k), 1.2, k)
    s.addPlane((0, 3, 0), (0, 1, 0), 0)
    return s


def _workload(case):
    if case not in _SCENES:
        cam = _camera(W, H)
        if case == "nested_glass":
            scene, _ = edge_scenes.get("nested_spheres")
        elif case == "glass_only":
            scene = _glass_only()
        elif case == "kinds_spheres":
            scene = _kinds_spheres()
        elif case == "mirrors_only":
            scene = _mirrors_only()
        else:
            wl = rt.workloads.get(case, width=W, height=H, **({"tex_size": 8} if case == "c3" else {}))
            scene, cam = wl.scene, wl.camera
        _SCENES[case] = (scene, cam)
    return _SCENES[case]


def _frame(t, cam, count, fused, calls=1):
    t.setOption(t.OPT_PREFIX_SHARING, 1 if fused else 0)
    t.setOption(t.OPT_SAMPLE_QUEUE, 1 if fused else 0)
    t.clear()
    for k in range(calls):
        t.renderSamples(cam, k * count, count)
    t.sync()
    return t.readLinear().copy()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _ran_the_changed_kernel(t, geom=0):
    """The last fused launch took pt_samples_q<COUNT = false, ACCEL = false, GEOM, ...>; GEOM 0: the instantiations that gather by use."""
    facts, plan = t.lastSamplePlan()
    return plan["family"] == A.PLAN_QUEUE and plan["accel"] == 0 and facts["count_enabled"] == 0 and plan["geom"] == geom


def _tracer(scene, w=W, h=H, arith="ieee"):
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    return t


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", SCENES)
def test_fused_frames_equal_the_direct_path(case, arith):
    scene, cam = _workload(case)
    t = _tracer(scene, arith=arith)
    try:
        for count in COUNTS:
            direct = _frame(t, cam, count, False)
            for tree in (0, 1):
                for fill in (0, 1):
                    t.setOption(t.OPT_PREFIX_TREE, tree)
                    t.setOption(t.OPT_WAVE_FILL, fill)
                    key = (case, arith, count, tree, fill)
                    assert _same(_frame(t, cam, count, True), direct), key
                    assert _ran_the_changed_kernel(t, 1 if case in MESHES else 0), key + (t.lastSamplePlan(),)
                    if count == 64:
                        assert t.lastSamplePlan()[1]["count_log2"] == 6, key
        assert t.walkOverflow() == 0
    finally:
        t.close()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", ["c2", "glass_only", "kinds_spheres"])
def test_two_calls_of_64_on_one_accumulator(case, arith):
    scene, cam = _workload(case)
    t = _tracer(scene, arith=arith)
    try:
        assert _same(_frame(t, cam, 64, True, calls=2), _frame(t, cam, 64, False, calls=2))
    finally:
        t.close()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case,k", [("c2", 16), ("glass_only", 32), ("kinds_spheres", 5)])
def test_render_again_served_from_look_ahead_frames(case, k, arith):
    """Every image after every call, against a context that runs the direct kernel on every call."""
    scene, cam = _workload(case)
    p = Pair(W, H, scene, arith, k)
    try:
        n = k + 2     # one whole batch and a part of the second
        p.render(cam, (case, k))
        p.renderAgain(cam, (case, k, arith), n)
        assert p.stats() == (2, n, 0, 0), (case, k)
    finally:
        p.close()


def _sparse_scene(w, h, live):
    """A light behind the eye and nothing in front of it (all sky), or one small diffuse sphere centred on the primary ray
    of pixel (20, 11), far smaller than the spacing of the pixels' rays there: one live pixel."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_DIFFUSE, (0.9, 0.5, 0.2), 1)
    s.addMaterial(A.T_LIGHT, (1, 1, 1), 0)
    s.addSphere((0, 0, -300), 100, 1)
    cam = _camera(w, h)
    if live:
        c = np.asarray(cam, dtype=np.float64)
        d = c[3:6] + (20.0 / w) * c[6:9] + (11.0 / h) * c[9:12]
        s.addSphere(tuple(float(v) for v in c[0:3] + d / np.linalg.norm(d) * 10.0), 0.05, 0)
    return s, cam


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("kind", ["one_live", "all_sky"])
def test_frames_with_next_to_no_live_pixel(kind, arith):
    scene, cam = _sparse_scene(48, 32, kind == "one_live")
    t = _tracer(scene, 48, 32, arith)
    try:
        for count in (8, 64, 65):
            direct = _frame(t, cam, count, False)
            assert _same(_frame(t, cam, count, True), direct), (kind, count)
            assert _ran_the_changed_kernel(t, 0), (kind, count)
            _, _, light, heavy = t.liveList()
            assert light + heavy == (1 if kind == "one_live" else 0), (kind, count, light, heavy)
    finally:
        t.close()


@pytest.mark.parametrize("arith", ARITHS)
def test_sharded_context_rank_1_of_3(arith):
    scene, cam = _workload("c2")
    t = _tracer(scene, arith=arith)
    t.setShard(1, 3)
    try:
        for count in (8, 64, 65):
            direct = _frame(t, cam, count, False)
            for fill in (0, 1):
                t.setOption(t.OPT_WAVE_FILL, fill)
                assert _same(_frame(t, cam, count, True), direct), (count, fill)
                assert _ran_the_changed_kernel(t, 0), (count, fill)
    finally:
        t.close()
