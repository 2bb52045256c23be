"""GPU (-m gpu): look-ahead for renderAgain (RT_OPT_LOOKAHEAD).  While the camera rests, one fused launch traces the next K
samples and replays the gamma-space running mean per pixel; the renderAgain calls hand the stored images out.  Every image
here is compared, bits with ==, after EVERY call against a second context that runs the direct kernel on every call
(RT_OPT_LOOKAHEAD 0) and goes through the same calls; rt_lookahead_stats proves that the batches happened, and that each
change that must drop the pending frames did."""
import os
import subprocess

import numpy as np
import pytest

import cases
from test_gpu_tree_fused import _glass_stack_scene

pytestmark = pytest.mark.gpu
rt = cases.rt


class Pair:
    """Two contexts over one scene: `on` looks K samples ahead, `off` never does.  do(f) applies f to both."""

    def __init__(self, w, h, scene, arith, k, fill=None):
        self.on = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
        self.off = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
        for t, v in ((self.on, k), (self.off, 0)):
            t.setArith(arith)
            if fill is not None:
                t.setOption(t.OPT_WAVE_FILL, fill)
            t.setOption(t.OPT_LOOKAHEAD, v)      # (explicit: the environment's RT_LOOKAHEAD must not matter here)
            t.setOption(t.OPT_PREFIX_CACHE, 1)   # (likewise RT_PREFIX_CACHE: the hit counts below assume the cache)
        self.again = 0

    def do(self, f):
        f(self.on)
        f(self.off)

    def stats(self):
        return self.on.lookaheadStats()

    def same(self, what=""):
        a, b = self.on.transferImage(), self.off.transferImage()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
        assert self.on.sample_counter == self.off.sample_counter, what
        return a

    def render(self, cam, what=""):
        self.do(lambda t: t.render(cam))
        self.again = 0
        return self.same((what, "render"))

    def renderAgain(self, cam, what="", n=1):
        img = None
        for _ in range(n):
            self.do(lambda t: t.renderAgain(cam))
            self.again += 1
            img = self.same((what, "renderAgain", self.again))
            assert self.on.sample_counter == self.again, what
        return img

    def close(self):
        off = self.off.lookaheadStats()
        for t in (self.on, self.off):
            assert t.walkOverflow() == 0
            t.close()
        assert off[0] == 0 and off[1] == 0 and off[3] == 0      # the comparison context never looked ahead


_WORKLOADS = {}


def _workload(name):
    if name not in _WORKLOADS:
        if name == "glass_stack":
            scene, cam = _glass_stack_scene()
            _WORKLOADS[name] = (scene, cam, 96, 54)
        else:
            kw = {"c2": dict(width=173, height=99),                                  # ragged; pt_samples_q with GEOM 0
                  "all_kinds": dict(width=200, height=120),                          # a lens, face-scanned meshes
                  "c3": dict(width=160, height=90, tex_size=64),                     # face records in LDS
                  "c5": dict(width=96, height=64, segments=24, rings=16),            # mesh BVH: pt_samples_w
                  "c4": dict(width=96, height=64, n_spheres=3000)}[name]             # sphere BVH
            wl = rt.workloads.get(name, **kw)
            _WORKLOADS[name] = (wl.scene, wl.camera, wl.width, wl.height)
    return _WORKLOADS[name]


# (K = 5: not a power of two, queue_fetch's multiply path; K >= 24: the shared decision trees are on)
@pytest.mark.parametrize("name,k", [("c2", 16), ("c2", 64), ("all_kinds", 5), ("c3", 2), ("c5", 5), ("c5", 16), ("c4", 16),
                                    ("glass_stack", 32), ("all_kinds", 32)])
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("arith", [0, 2])
def test_sequence_equals_the_direct_kernel(name, k, fill, arith):
    scene, cam, w, h = _workload(name)
    p = Pair(w, h, scene, arith, k, fill=fill)
    try:
        n = 2 * k + max(1, min(3, k - 1))     # two whole batches and a part of the third
        p.render(cam, (name, k))
        img = p.renderAgain(cam, (name, k, fill, arith), n)
        assert np.isfinite(img).all() and img[..., :3].sum() > 0 and (img[..., 3] == 1).all()
        batches, served, direct, discarded = p.stats()
        assert (batches, served, direct, discarded) == (3, n, 0, 0), (name, k)
        # the launches went through the fused path's prefix cache: traced once, reused twice
        assert p.on.prefixCacheStats() == (2, 1)
    finally:
        p.close()


def _sparse_scene(n_spheres):
    """The scenes of test_live_list_far_shorter_than_the_grid: no live pixel at all / a single one."""
    s = rt.SceneCreator()
    s.addMaterial(rt._abi.T_DIFFUSE, (0.9, 0.5, 0.2), 1)
    s.addMaterial(rt._abi.T_LIGHT, (1, 1, 1), 0)
    s.addSphere((0, 0, -300), 100, 1)
    if n_spheres:
        s.addSphere((0.0, 0.0, 100.0), 0.3, 0)
    return s, rt.Camera(60, 1.0, (0, 0, 0), 0.0, 0.0).transferData()


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("kind", ["empty", "all_sky", "one_live", "1x1"])
def test_frames_with_next_to_no_live_pixel(kind, arith):
    if kind == "empty":
        scene = rt.SceneCreator()
        scene.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
        cam, w, h = rt.Camera(60, 33 / 17).transferData(), 33, 17
    elif kind == "1x1":
        scene, cam, _, _ = _workload("all_kinds")
        w, h = 1, 1
    else:
        scene, cam = _sparse_scene(1 if kind == "one_live" else 0)
        w, h = 128, 128
    p = Pair(w, h, scene, arith, 4)
    try:
        p.render(cam, kind)
        p.renderAgain(cam, kind, 10)
        assert p.stats() == (3, 10, 0, 0)
    finally:
        p.close()


def test_every_image_equals_the_cpu_oracle(oracle, table):
    wl = rt.workloads.get("all_kinds", width=40, height=24)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setOption(t.OPT_LOOKAHEAD, 8)
        ref, _ = oracle.render(wl.scene, wl.camera, table, wl.width, wl.height, 0, threads=8)
        t.render(wl.camera)
        assert np.array_equal(t.transferImage().view(np.uint32), ref.view(np.uint32))
        for s in range(1, 21):
            ref, _ = oracle.render(wl.scene, wl.camera, table, wl.width, wl.height, 1, first=s, image=ref, threads=8)
            t.renderAgain(wl.camera)
            assert np.array_equal(t.transferImage().view(np.uint32), ref.view(np.uint32)), "retrace %d" % s
        assert t.lookaheadStats() == (3, 20, 0, 0)
    finally:
        t.close()


def test_stats_count_batches_served_and_dropped_frames():
    scene, cam, w, h = _workload("c2")
    p = Pair(w, h, scene, 0, 4)
    try:
        assert p.stats() == (0, 0, 0, 0)
        p.render(cam)
        p.renderAgain(cam, "stats", 9)
        assert p.stats() == (3, 9, 0, 0)
        assert p.off.lookaheadStats() == (0, 0, 9, 0)
        p.render(cam)
        assert p.stats() == (3, 9, 0, 3)          # the third batch's other three frames
        assert p.off.lookaheadStats() == (0, 0, 9, 0)
        # option values the option refuses; 0 switches it off and back
        for bad in (1, 65, -2):
            with pytest.raises(rt.RtError):
                p.on.setOption(p.on.OPT_LOOKAHEAD, bad)
        p.on.setOption(p.on.OPT_LOOKAHEAD, 0)
        p.renderAgain(cam, "off", 3)
        assert p.stats() == (3, 9, 3, 3)
        p.on.setOption(p.on.OPT_LOOKAHEAD, 6)     # (a larger ring than before)
        p.renderAgain(cam, "on again", 7)
        assert p.stats() == (5, 16, 3, 3)
    finally:
        p.close()


def _ulp_up(cam, i):
    c = np.array(cam, dtype=np.float32)
    c[i] = np.nextafter(c[i], np.float32(np.inf))
    return c


@pytest.mark.parametrize("arith", [0, 2])
def test_every_change_drops_the_pending_frames(arith):
    """In the middle of a batch one thing changes at a time, on both contexts.  The next three images must equal the
    comparison context's, and the frames computed before the change must have been dropped."""
    wl = rt.workloads.get("all_kinds", width=120, height=72)
    cam, scene = wl.camera, wl.scene
    other = rt.workloads.get("c2", width=120, height=72).scene
    cam2 = _ulp_up(cam, 4)
    p = Pair(wl.width, wl.height, scene, arith, 8)
    try:
        def settle():
            """render + 3 renderAgain: a batch of 8 has been launched and 5 of its frames are pending"""
            b0 = p.stats()[0]
            p.render(cam, "settle")
            p.renderAgain(cam, "settle", 3)
            b, _, _, d = p.stats()
            assert b == b0 + 1
            return p.stats()

        def after(what, before, camera=cam, direct=False):
            p.renderAgain(camera, what, 3)
            b, s, dr, d = p.stats()
            assert d >= before[3] + 5, (what, before, (b, s, dr, d))
            if direct:
                assert dr >= before[2] + 3 and b == before[0], (what, before, (b, s, dr, d))
            else:
                assert b == before[0] + 1, (what, before, (b, s, dr, d))

        # another camera in renderAgain: that call runs the direct kernel, the next one starts a batch
        st = settle()
        p.renderAgain(cam2, "camera")
        b, s, dr, d = p.stats()
        assert (b, s, dr, d) == (st[0], st[1], st[2] + 1, st[3] + 5)
        p.renderAgain(cam2, "camera", 2)
        assert p.stats() == (st[0] + 1, st[1] + 2, st[2] + 1, st[3] + 5)
        # render
        st = settle()
        p.render(cam, "render")
        after("render", st)
        # the fused path writes the image through resolve
        st = settle()

        def fused(t):
            t.clear()
            t.renderSamples(cam, 0, 8)
            t.resolve()
        p.do(fused)
        p.same("resolve")
        after("resolve", st)
        # the seed
        st = settle()
        p.do(lambda t: t.setSeed(12345))
        after("seed", st)
        p.do(lambda t: t.setSeed(cases.SEED))
        # an option
        st = settle()
        p.do(lambda t: t.setOption(t.OPT_ACCEL, 0))
        after("option", st)
        p.do(lambda t: t.setOption(t.OPT_ACCEL, 1))
        # a new scene
        st = settle()
        p.do(lambda t: t.setScene(other))
        p.again = 0                                   # (rt_set_scene resets the sample counter)
        after("scene", st)
        p.do(lambda t: t.setScene(scene))
        # the frame size
        st = settle()
        p.do(lambda t: t.resize(wl.width + 8, wl.height))
        p.again = 0
        after("resize", st)
        p.do(lambda t: t.resize(wl.width, wl.height))
        # the policy
        st = settle()
        p.do(lambda t: t.setArith(2 - arith))
        p.again = 0                                   # (so does RT_OPT_ARITH)
        after("policy", st)
        p.do(lambda t: t.setArith(arith))
        # a shard: sharded contexts run the direct kernel
        st = settle()
        p.do(lambda t: t.setShard(0, 2, 8, 8))
        after("shard", st, direct=True)
        assert p.on.counters().as_dict() == p.off.counters().as_dict()
        p.do(lambda t: t.setShard(0, 1, 8, 8))
        # counters: the counting kernels are the direct ones
        st = settle()

        def counting(t):
            t.enableCounters(True)
            t.resetCounters()
        p.do(counting)
        after("counters", st, direct=True)
        cn = p.on.counters().as_dict()
        assert cn == p.off.counters().as_dict() and cn["samples"] == 3 * wl.width * wl.height
        p.do(lambda t: t.enableCounters(False))
        # and what needs the fused path's pieces runs direct without them
        for opt in (p.on.OPT_PREFIX_SHARING, p.on.OPT_SAMPLE_QUEUE):
            st = settle()
            p.do(lambda t: t.setOption(opt, 0))
            after(("off", opt), st, direct=True)
            p.do(lambda t: t.setOption(opt, 1))
        st = settle()
        p.do(lambda t: t.setOption(t.OPT_MAX_THREADS_PER_LAUNCH, 4096))
        after("several slot ranges", st, direct=True)
        p.do(lambda t: t.setOption(t.OPT_MAX_THREADS_PER_LAUNCH, 1 << 30))
        settle()
    finally:
        p.close()


@pytest.mark.parametrize("arith", [0, 2])
def test_nothing_else_moves(arith):
    scene, cam, w, h = _workload("all_kinds")
    p = Pair(w, h, scene, arith, 4)
    try:
        def fused(t):
            t.clear()
            t.renderSamples(cam, 0, 8)
        p.do(fused)
        acc = p.on.readLinear()
        assert np.array_equal(acc.view(np.uint32), p.off.readLinear().view(np.uint32))
        p.render(cam)
        p.renderAgain(cam, "accumulator", 6)
        assert p.stats()[0] == 2
        assert np.array_equal(p.on.readLinear().view(np.uint32), acc.view(np.uint32))      # look-ahead launches add nothing
        # the prefix-cache entry a look-ahead launch leaves serves the fused path: same accumulator as without
        hits = p.on.prefixCacheStats()[0]
        p.do(fused)
        assert p.on.prefixCacheStats()[0] == hits + 1
        assert np.array_equal(p.on.readLinear().view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(p.off.readLinear().view(np.uint32), acc.view(np.uint32))
        # and the image still continues where it was
        p.renderAgain(cam, "after the fused call", 3)
    finally:
        p.close()


def test_one_history_entry_per_call():
    scene, cam, w, h = _workload("c2")
    cam2 = _ulp_up(cam, 0)
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    try:
        t.setOption(t.OPT_LOOKAHEAD, 4)
        t.render(cam)
        assert len(t.kernelMsHistory()) == 1
        for i in range(10):                      # batch, served, served, served, batch, ...
            t.renderAgain(cam)
            assert len(t.kernelMsHistory()) == 2 + i
        t.renderAgain(cam2)                      # direct
        assert len(t.kernelMsHistory()) == 12
        assert t.lookaheadStats() == (3, 10, 1, 2)
        first, second = t.stageMsHistory()
        assert len(first) == len(second) == 12 and all(v >= 0 for v in first + second)
        ms = t.kernelMsHistory()
        assert all(v > 0 for v in ms)
    finally:
        t.close()


def test_cli_progressive_lookahead_writes_the_same_file(built, tmp_path):
    cli = os.path.join(cases.ROOT, "host", "rt_cli")
    out = {}
    for k in (8, 0):
        tga = str(tmp_path / ("k%d.tga" % k))
        subprocess.run([cli, "--scene", os.path.join(cases.ROOT, "assets", "scenes", "all_kinds.scene"), "--size", "64x40",
                        "--spp", "20", "--camera=-8,-1,-8,45,0", "--progressive", "--lookahead", str(k), "--out", tga],
                       check=True, cwd=cases.ROOT)
        out[k] = open(tga, "rb").read()
    assert len(out[8]) == 18 + 3 * 64 * 40 and out[8] == out[0]
    # the flag belongs to --progressive, and 1 is no batch size
    for bad in (["--lookahead", "8"], ["--progressive", "--lookahead", "1"]):
        r = subprocess.run([cli, "--scene", os.path.join(cases.ROOT, "assets", "scenes", "all_kinds.scene")] + bad,
                           cwd=cases.ROOT, capture_output=True)
        assert r.returncode == 2
