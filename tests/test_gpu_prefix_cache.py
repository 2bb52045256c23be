"""GPU (-m gpu): the prefix cache (RT_OPT_PREFIX_CACHE).  While the camera block, the scene and every setting stay as
they are, a fused call keeps what pt_prefix left in the context and only replays the finished pixels' sums
(pt_final_replay) before the sample kernel.  Every frame here is compared, accumulator bits with ==, against a second
context that traces the prefix on every call (RT_OPT_PREFIX_CACHE 0) and goes through the same calls; rt_prefix_cache_stats
proves that the hits happened, and that each change that must invalidate the entry did."""
import ctypes as C

import numpy as np
import pytest

import cases
from test_gpu_tree_fused import _glass_stack_scene

pytestmark = pytest.mark.gpu
rt = cases.rt


class Pair:
    """Two contexts over one scene: `on` keeps the prefix, `off` traces it on every call.  do(f) applies f to both."""

    def __init__(self, w, h, scene, arith, fill=None, shard=None):
        self.on = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
        self.off = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
        for t, cache in ((self.on, 1), (self.off, 0)):
            t.setArith(arith)
            if fill is not None:
                t.setOption(t.OPT_WAVE_FILL, fill)
            if shard is not None:
                t.setShard(*shard)
            t.setOption(t.OPT_PREFIX_CACHE, cache)      # (explicit: the environment's RT_PREFIX_CACHE must not matter here)
        self.base = self.stats()

    def do(self, f):
        f(self.on)
        f(self.off)

    def render(self, cam, first, spp, clear=True):
        def f(t):
            if clear:
                t.clear()
            t.renderSamples(cam, first, spp)
        self.do(f)

    def stats(self):
        return self.on.prefixCacheStats()

    def since(self):
        """(hits, misses) of the caching context since the last call of since() (or since the pair was made)."""
        h, m = self.stats()
        d = (h - self.base[0], m - self.base[1])
        self.base = (h, m)
        return d

    def same(self, what=""):
        self.do(lambda t: t.sync())
        a, b = self.on.readLinear(), self.off.readLinear()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
        return a

    def close(self):
        off_hits = self.off.prefixCacheStats()[0]
        for t in (self.on, self.off):
            assert t.walkOverflow() == 0
            t.close()
        assert off_hits == 0        # the comparison context never reused anything


def _workload(name):
    if name == "c2":
        wl = rt.workloads.get("c2")
        return wl.scene, wl.camera, wl.width, wl.height
    if name == "c5":
        wl = rt.workloads.get("c5", width=320, height=180)
        return wl.scene, wl.camera, wl.width, wl.height
    if name == "all_kinds":
        wl = rt.workloads.get("all_kinds", width=300, height=200)
        return wl.scene, wl.camera, wl.width, wl.height
    scene, cam = _glass_stack_scene()
    return scene, cam, 320, 180


@pytest.fixture(scope="module", params=["c2", "c5", "all_kinds", "glass_stack"])
def workload(request):
    return (request.param,) + _workload(request.param)


@pytest.mark.parametrize("arith", [0, 2])
def test_hits_equal_a_fresh_trace(workload, arith):
    name, scene, cam, w, h = workload
    p = Pair(w, h, scene, arith)
    try:
        # the same frame three times: traced once, reused twice
        for k in range(3):
            p.render(cam, 0, 64)
            img = p.same((name, arith, "repeat", k))
        assert p.since() == (2, 1), (name, arith)
        assert np.isfinite(img).all() and img[..., :3].sum() > 0
        # progressive, no clear in between: the closed form at other counts and another lane-group size
        p.do(lambda t: t.clear())
        for first, n in ((0, 64), (64, 64), (128, 40), (168, 100)):
            p.render(cam, first, n, clear=False)
            p.same((name, arith, "progressive", first, n))
        assert p.since() == (4, 0), (name, arith)
        assert (p.on.sampleCounts() == 268).all()
        # one call of 1024 spp runs as two launches of 512: the first traces (an option was set in between), the
        # second reuses the first's prefix
        p.do(lambda t: t.setOption(t.OPT_PREFIX_TREE, 1))
        p.render(cam, 0, 1024)
        p.same((name, arith, "1024"))
        assert p.since() == (1, 1), (name, arith)
    finally:
        p.close()


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("n_spheres", [0, 1])
def test_all_sky_and_one_live_pixel(n_spheres, arith):
    """The scenes of test_live_list_far_shorter_than_the_grid: no live pixel at all / a single one out of 65 536."""
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (0.9, 0.5, 0.2), 1)
    s.addMaterial(rt._abi.T_LIGHT, (1, 1, 1), 0)
    s.addSphere((0, 0, -300), 100, 1)
    if n_spheres:
        s.addSphere((0.0, 0.0, 100.0), 0.3, 0)
    cam = rt.Camera(60, 1.0, (0, 0, 0), 0.0, 0.0).transferData()
    p = Pair(256, 256, s, arith)
    try:
        for k in range(3):
            p.render(cam, 0, 64)
            p.same((n_spheres, arith, k))
        p.render(cam, 64, 37, clear=False)
        p.same((n_spheres, arith, "more"))
        assert p.since() == (3, 1)
        assert (p.on.sampleCounts() == 101).all()
        # small counts (groups of 8 and 4 lanes) are hits only where they leave the same records: trees in every call
        p.do(lambda t: t.setOption(t.OPT_PREFIX_TREE, 2))
        for first, n in ((0, 64), (64, 5), (69, 3)):
            p.render(cam, first, n, clear=first == 0)
            p.same((n_spheres, arith, "small", n))
        assert p.since() == (2, 1)
    finally:
        p.close()


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("fill", [0, 1])
def test_sharded_context(fill, arith):
    """Rank 1 of 3: the slots are this rank's tiles only, and the replay must find their pixels again."""
    wl = rt.workloads.get("c2", width=640, height=360)
    p = Pair(wl.width, wl.height, wl.scene, arith, fill=fill, shard=(1, 3, 8, 8))
    try:
        for k in range(3):
            p.render(wl.camera, 0, 64)
            p.same((fill, arith, k))
        p.render(wl.camera, 64, 24, clear=False)
        p.same((fill, arith, "more"))
        assert p.since() == (3, 1)
        counts = p.on.sampleCounts()
        owned = counts != 0
        assert 0.3 < owned.mean() < 0.37 and (counts[owned] == 88).all()
    finally:
        p.close()


def _ulp_up(cam, i):
    c = np.array(cam, dtype=np.float32)
    c[i] = np.nextafter(c[i], np.float32(np.inf))
    return c


@pytest.mark.parametrize("arith", [0, 2])
def test_every_change_invalidates(arith):
    """Between two otherwise equal calls one thing changes at a time.  The frame must equal the comparison context's every
    time, and where the kept prefix no longer describes the call the miss count must have grown."""
    wl = rt.workloads.get("all_kinds", width=300, height=200)
    cam, scene = wl.camera, wl.scene
    other = rt.workloads.get("c2").scene
    other_arith = 2 - arith
    p = Pair(wl.width, wl.height, scene, arith)
    try:
        def settle():
            """two equal calls: whatever came before, the second one must be a hit"""
            p.render(cam, 0, 64)
            p.same("settle 1")
            p.since()
            p.render(cam, 0, 64)
            p.same("settle 2")
            assert p.since() == (1, 0)

        def expect_miss(what, camera=cam, spp=64):
            p.render(camera, 0, spp)
            p.same(what)
            hits, misses = p.since()
            assert misses >= 1 and hits == 0, (what, hits, misses)

        settle()
        # the camera, by one ulp in one float (and back)
        for i in (0, 4, 11):
            expect_miss(("camera", i), _ulp_up(cam, i))
            expect_miss(("camera back", i))
        # the scene
        settle()
        p.do(lambda t: t.setScene(other))
        expect_miss("scene")
        p.do(lambda t: t.setScene(scene))
        expect_miss("scene back")
        # the textures alone
        settle()
        tex = np.ascontiguousarray(scene.textures[:, ::-1, ::-1] * np.float32(0.5))
        layers, th, tw, _ = tex.shape
        p.do(lambda t: t._check(t._lib.rt_set_textures(t._ctx, tex.ctypes.data_as(C.c_void_p), tw, th, layers)))
        expect_miss("textures")
        p.do(lambda t: t.setScene(scene))
        # the seed
        settle()
        p.do(lambda t: t.setSeed(12345))
        expect_miss("seed")
        p.do(lambda t: t.setSeed(cases.SEED))
        # the policy
        settle()
        p.do(lambda t: t.setArith(other_arith))
        expect_miss("policy")
        p.do(lambda t: t.setArith(arith))
        expect_miss("policy back")
        # options
        for opt, value, back in ((p.on.OPT_ACCEL, 0, 1), (p.on.OPT_PREFIX_TREE, 0, 1), (p.on.OPT_PREFIX_TREE, 2, 1)):
            settle()
            p.do(lambda t: t.setOption(opt, value))
            expect_miss(("option", opt, value))
            p.do(lambda t: t.setOption(opt, back))
            expect_miss(("option back", opt))
        # the shard
        settle()
        p.do(lambda t: t.setShard(1, 2, 8, 8))
        expect_miss("shard")
        p.do(lambda t: t.setShard(0, 1, 8, 8))
        expect_miss("shard back")
        # the frame size
        settle()
        p.do(lambda t: t.resize(wl.width + 8, wl.height))
        expect_miss("frame size")
        p.do(lambda t: t.resize(wl.width, wl.height))
        expect_miss("frame size back")
        # the stream
        import torch
        settle()
        stream = torch.cuda.Stream()
        p.do(lambda t: t.setStream(stream.cuda_stream))
        expect_miss("stream")
        p.do(lambda t: t.setStream(0))
        expect_miss("stream back")
        # several slot ranges per frame: every such launch takes the full path and keeps nothing
        settle()
        p.do(lambda t: t.setOption(t.OPT_MAX_THREADS_PER_LAUNCH, 1 << 16))
        expect_miss("two ranges")
        expect_miss("two ranges again")
        p.do(lambda t: t.setOption(t.OPT_MAX_THREADS_PER_LAUNCH, 1 << 30))
        expect_miss("one range again")
        # counters on (the counting kernels run) and off again
        settle()
        p.do(lambda t: t.enableCounters(True))
        expect_miss("counters on")
        expect_miss("counters still on")
        p.do(lambda t: t.enableCounters(False))
        expect_miss("counters off")
        # an adaptive render in between: its masked rounds write the slot buffers for their blocks only
        settle()
        stats = []
        p.do(lambda t: stats.append(t.renderAdaptive(cam, 2e-3, batch=32, min_spp=64, max_spp=256, block=(8, 8))))
        assert stats[0] == stats[1]
        p.same("adaptive")
        assert np.array_equal(p.on.sampleCounts(), p.off.sampleCounts())
        p.since()
        expect_miss("after adaptive")
        # probes in between touch nothing the prefix lives in: the next call reuses it
        settle()
        xs, ys, ss = np.arange(50) % wl.width, np.arange(50) % wl.height, np.arange(50) % 64
        got = []
        p.do(lambda t: got.append(t.traceSamples(cam, xs, ys, ss)))
        assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
        p.since()
        p.render(cam, 0, 64)
        p.same("after traceSamples")
        assert p.since() == (1, 0)      # probes do not invalidate
        # 8 spp (no decision trees) and 64 spp (trees) leave different records
        settle()
        expect_miss("8 spp", spp=8)
        expect_miss("64 spp after 8")
        # and with the cache switched off on the caching context nothing is reused
        settle()
        p.on.setOption(p.on.OPT_PREFIX_CACHE, 0)
        expect_miss("cache off")
        expect_miss("cache off again")
        p.on.setOption(p.on.OPT_PREFIX_CACHE, 1)
        settle()
    finally:
        p.close()
