"""GPU (-m gpu): the sample kernels' grid (RT_OPT_EXACT_GRID).  A workgroup of pt_samples_q / pt_samples_w / pt_samples
that owns no pixel leaves before it stages anything, and while a fused call reuses the kept prefix the host learns the
length of the live list (one asynchronous copy, enqueued by the first hit) and launches exactly the workgroups that own a
pixel.  Every frame here is compared, accumulator bits with ==, against a second context with RT_OPT_EXACT_GRID 0 that goes
through the same calls; rt_sample_grid_stats proves which launches were exact, and rt_debug_live_list + rt_sample_units say
how many workgroups such a launch must have had."""
import numpy as np
import pytest

import cases
from test_gpu_tree_fused import _glass_stack_scene

pytestmark = pytest.mark.gpu
rt = cases.rt


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Pair:
    """Two contexts over one scene, both keeping the prefix: `on` sizes its hits by the live list, `off` never does."""

    def __init__(self, w, h, scene, arith, fill=None, shard=None, queue=None):
        self.on = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
        self.off = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
        for t, exact in ((self.on, 1), (self.off, 0)):
            t.setArith(arith)
            if fill is not None:
                t.setOption(t.OPT_WAVE_FILL, fill)
            if queue is not None:
                t.setOption(t.OPT_SAMPLE_QUEUE, queue)
            if shard is not None:
                t.setShard(*shard)
            t.setOption(t.OPT_PREFIX_CACHE, 1)          # (explicit: the environment must not matter here)
            t.setOption(t.OPT_EXACT_GRID, exact)
        self.base = self.on.sampleGridStats()

    def do(self, f):
        f(self.on)
        f(self.off)

    def render(self, cam, first, spp, clear=True):
        def f(t):
            if clear:
                t.clear()
            t.renderSamples(cam, first, spp)
        self.do(f)

    def since(self):
        """(launches, exact launches, workgroups) of the exact-grid context since the last call of since()."""
        s = self.on.sampleGridStats()
        d = tuple(s[i] - self.base[i] for i in range(3))
        self.base = s
        return d

    def same(self, what=""):
        self.do(lambda t: t.sync())
        a, b = self.on.readLinear(), self.off.readLinear()
        assert np.array_equal(_bits(a), _bits(b)), what
        return a

    def close(self):
        off_exact = self.off.sampleGridStats()[1]
        for t in (self.on, self.off):
            assert t.walkOverflow() == 0
            t.close()
        assert off_exact == 0       # the comparison context never had an exact grid


def _group_log2(spp):
    g = 0
    while (1 << g) < spp and g < 6:
        g += 1
    return g


def _sequence(p, cam, spp, what, fixed=False):
    """miss, hit, sync, hit: the third render's launches (one per 512 samples) are exact and have the host function's
    number of workgroups for the counts read back from the device.  → (units, light count, heavy count)."""
    per_call = (spp + 511) // 512
    p.since()
    p.render(cam, 0, spp)                   # traces the prefix (a call of 1024: its second launch already hits)
    p.same((what, "miss"))
    launches, exact, wg_worst = p.since()
    assert (launches, exact) == (per_call, 0), what
    p.render(cam, 0, spp)                   # a hit: the copy of the counters is under way (1024: known by its second launch)
    p.same((what, "hit"))                   # (synchronises)
    p.since()
    p.render(cam, 0, spp)
    img = p.same((what, "exact"))
    launches, exact, wg = p.since()
    assert (launches, exact) == (per_call, per_call), what
    cap, per, light, heavy = p.on.liveList()
    units = rt.sample_units(cap, per, light, heavy)
    print("%s: cap %d, %d per unit, light %d heavy %d -> %d units (worst case %d)" %
          (what, cap, per, light, heavy, units, -(-cap // per) + 1))
    expect = units
    if fixed:                               # the fixed-lane kernel: pixel groups of 2^g lanes in workgroups of 256
        assert per == 1
        expect = ((units << _group_log2(min(spp, 512))) + 255) // 256
    assert wg == per_call * expect, what
    assert p.on.sampleGridStats()[3] == expect
    assert wg <= wg_worst
    assert np.isfinite(img).all()
    return units, light, heavy


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("spp", [1, 5, 64, 200, 1024])
def test_c2_sequence(spp, arith):
    wl = rt.workloads.get("c2", width=96, height=54)
    p = Pair(wl.width, wl.height, wl.scene, arith)
    try:
        units, light, heavy = _sequence(p, wl.camera, spp, ("c2", spp, arith))
        assert 0 < light + heavy < wl.width * wl.height and units > 0
        # more samples into the same accumulator: still exact, still equal
        p.render(wl.camera, spp, min(spp, 512), clear=False)
        p.same(("c2 more", spp, arith))
        assert p.since()[:2] == (1, 1)
    finally:
        p.close()


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("n_spheres", [0, 1])
def test_all_sky_and_one_live_pixel(n_spheres, arith):
    """No live pixel at all — the sample kernel is not launched — and a single one out of 4 096."""
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (0.9, 0.5, 0.2), 1)
    s.addMaterial(rt._abi.T_LIGHT, (1, 1, 1), 0)
    s.addSphere((0, 0, -300), 100, 1)
    if n_spheres:
        s.addSphere((0.0, 0.0, 100.0), 1.2, 0)      # on the axis: pixel (32, 32) looks straight at it, its neighbours pass beside it
    cam = rt.Camera(60, 1.0, (0, 0, 0), 0.0, 0.0).transferData()
    for queue in (1, 0):
        p = Pair(64, 64, s, arith, queue=queue)
        try:
            units, light, heavy = _sequence(p, cam, 64, ("sky", n_spheres, arith, queue), fixed=not queue)
            assert light + heavy == n_spheres and units == n_spheres
            assert (p.on.sampleCounts() == 64).all()
        finally:
            p.close()


@pytest.mark.parametrize("arith", [0, 2])
def test_nested_glass_has_both_parts(arith):
    scene, cam = _glass_stack_scene()
    p = Pair(96, 54, scene, arith)
    try:
        units, light, heavy = _sequence(p, cam, 64, ("glass", arith))
        assert light > 0 and heavy > 0
    finally:
        p.close()


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("case", ["all_kinds", "c5", "fill0", "fill1", "fixed", "shard"])
def test_other_kernels_and_modes(case, arith):
    kw, fixed = {}, False
    if case == "all_kinds":                 # GEOM 1
        wl = rt.workloads.get("all_kinds", width=64, height=48)
    elif case == "c5":                      # pt_samples_w
        wl = rt.workloads.get("c5", width=32, height=18)
    else:
        wl = rt.workloads.get("c2", width=96, height=54)
        if case in ("fill0", "fill1"):
            kw = dict(fill=int(case[-1]))
        elif case == "fixed":               # the sample queue off: pt_samples
            kw, fixed = dict(queue=0), True
        else:                               # rank 1 of 3
            kw = dict(shard=(1, 3, 8, 8))
    p = Pair(wl.width, wl.height, wl.scene, arith, **kw)
    try:
        units, light, heavy = _sequence(p, wl.camera, 64, (case, arith), fixed=fixed)
        assert units > 0
    finally:
        p.close()


def _fresh(w, h, scene, arith, cam, spp, seed=cases.SEED):
    t = rt.RayTracer(w, h, scene=scene, seed=seed)
    try:
        t.setArith(arith)
        t.setOption(t.OPT_EXACT_GRID, 0)
        t.clear()
        t.renderSamples(cam, 0, spp)
        t.sync()
        return t.readLinear()
    finally:
        t.close()


@pytest.mark.parametrize("arith", [0, 2])
def test_every_change_drops_the_counts(arith):
    """Between two hits one thing changes: the next launch has the worst-case grid again, and the frame equals a fresh
    context's.  A stale count (or anything else kept per scene and policy) would show in one of the two."""
    wl = rt.workloads.get("c2", width=96, height=54)
    w, h, cam, scene = wl.width, wl.height, wl.camera, wl.scene
    other = rt.SceneCreator()                       # other materials, other geometry, far fewer live pixels
    other.addMaterial(rt._abi.T_DIELECTRIC, (1, 0.9, 0.8), 1.7)
    other.addMaterial(rt._abi.T_DIFFUSE, (0.2, 0.7, 0.9), 1)
    other.addMaterial(rt._abi.T_LIGHT, (1, 1, 1), 0)
    other.addSphere((0, -300, 0), 150, 2)
    other.addSphere((-8 + 1.5, -1 + 0.5, -8 + 1.5), 0.6, 0)
    other.addSphere((-8 + 3.0, -1.5, -8 + 3.0), 0.9, 1)
    p = Pair(w, h, scene, arith)
    try:
        def settle(camera=cam):
            _sequence(p, camera, 64, "settle")

        def expect_worst(what, ref_scene, ref_arith, ref_size=(w, h), seed=cases.SEED):
            p.since()
            p.render(cam, 0, 64)
            img = p.same(what)
            launches, exact, wg = p.since()
            cap, per, _, _ = p.on.liveList()
            assert (launches, exact, wg) == (1, 0, -(-cap // per) + 1), what     # ("every pixel is live")
            ref = _fresh(ref_size[0], ref_size[1], ref_scene, ref_arith, cam, 64, seed)
            assert np.array_equal(_bits(img), _bits(ref)), what

        settle()
        p.do(lambda t: t.setScene(other))
        expect_worst("scene", other, arith)
        settle()
        p.do(lambda t: t.setScene(scene))
        expect_worst("scene back", scene, arith)
        settle()
        p.do(lambda t: t.setArith(2 - arith))
        expect_worst("policy", scene, 2 - arith)
        settle()
        p.do(lambda t: t.setArith(arith))
        expect_worst("policy back", scene, arith)
        settle()
        p.do(lambda t: t.setSeed(12345))
        expect_worst("seed", scene, arith, seed=12345)
        p.do(lambda t: t.setSeed(cases.SEED))
        settle()
        p.do(lambda t: t.resize(w + 8, h))
        expect_worst("frame size", scene, arith, ref_size=(w + 8, h))
        p.do(lambda t: t.resize(w, h))
        settle()
        # the option itself: off means the worst-case grid on a hit too, on again means learning the counts anew
        p.on.setOption(p.on.OPT_EXACT_GRID, 0)
        p.render(cam, 0, 64)
        p.render(cam, 0, 64)
        p.same("option off")
        assert p.since()[:2] == (2, 0)
        p.on.setOption(p.on.OPT_EXACT_GRID, 1)
        settle()
    finally:
        p.close()
