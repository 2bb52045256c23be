"""GPU (-m gpu): progressive anti-aliasing — rt_render_again_cameras, renderAgain through a cyclic schedule of camera blocks,
with look-ahead through the table.  The call that makes sample s looks through block s mod n.  Every image here is compared,
bits with ==, after EVERY call: a context with RT_OPT_LOOKAHEAD K against one with 0, both going through the same calls
(tests/test_gpu_lookahead.py's Pair), and — the schedule rule — against a third context that calls renderAgain with the
block written out.  rt_lookahead_stats proves that the batches happened and that each change that must drop the pending
frames did."""
import os
import subprocess

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
rt = cases.rt
T = rt.RayTracer
QUEUE = rt._abi.CAMERA_PLAN_QUEUE
EINVAL, ESTATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def table_of(block, n, w, h):
    """n camera blocks about `block` (position, lower-left corner, horizontal, vertical): Camera.sampleBlocks' offsets — a
    jitter inside the pixel and a small lens — applied to a block instead of a Camera, so that every workload has a table."""
    block = np.asarray(block, np.float32)
    pos, llc, hor, ver = block[0:3], block[3:6], block[6:9], block[9:12]
    off = rt.Camera.sampleOffsets(n)
    out = np.empty((n, 12), np.float32)
    for j in range(n):
        dx, dy, lx, ly = off[j]
        lens = np.float32(0.01) * (lx * hor + ly * ver)
        out[j] = np.concatenate([pos + lens, llc + (dx / np.float32(w)) * hor + (dy / np.float32(h)) * ver - lens, hor, ver])
    assert len({r.tobytes() for r in out}) == n
    return out


_WORKLOADS = {}


def _workload(name):
    if name not in _WORKLOADS:
        kw = {"c2": dict(width=173, height=99),                                  # ragged: waves whose slots leave the frame; GEOM 0
              "all_kinds": dict(width=200, height=120),                          # a lens, face-scanned meshes
              "c3": dict(width=160, height=90, tex_size=64),                     # face records in LDS
              "c5": dict(width=96, height=64, segments=24, rings=16),            # mesh BVH: the (1, 2) row
              "c4": dict(width=96, height=64, n_spheres=3000)}[name]             # sphere BVH
        wl = rt.workloads.get(name, **kw)
        _WORKLOADS[name] = (wl.scene, wl.camera, wl.width, wl.height)
    return _WORKLOADS[name]


class Pair:
    """Two contexts over one scene: `on` looks K samples ahead, `off` never does.  do(f) applies f to both."""

    def __init__(self, w, h, scene, arith, k, fill=None, accel=None):
        self.on = T(w, h, scene=scene, seed=cases.SEED)
        self.off = T(w, h, scene=scene, seed=cases.SEED)
        for t, v in ((self.on, k), (self.off, 0)):
            t.setArith(arith)
            if fill is not None:
                t.setOption(t.OPT_WAVE_FILL, fill)
            if accel is not None:
                t.setOption(t.OPT_ACCEL, accel)
            t.setOption(t.OPT_LOOKAHEAD, v)      # (explicit: the environment's RT_LOOKAHEAD must not matter here)
            t.setOption(t.OPT_PREFIX_CACHE, 1)
        self.counter = 0

    def do(self, f):
        f(self.on)
        f(self.off)

    def stats(self):
        return self.on.lookaheadStats()

    def same(self, what=""):
        a, b = self.on.transferImage(), self.off.transferImage()
        assert np.array_equal(bits(a), bits(b)), what
        assert self.on.sample_counter == self.off.sample_counter == self.counter, what
        return a

    def render(self, cam, what=""):
        self.do(lambda t: t.render(cam))
        self.counter = 0
        return self.same((what, "render"))

    def renderAgain(self, cam, what="", n=1):
        for _ in range(n):
            self.do(lambda t: t.renderAgain(cam))
            self.counter += 1
            self.same((what, "renderAgain", self.counter))

    def cameras(self, table, what="", n=1):
        img = None
        for _ in range(n):
            self.do(lambda t: t.renderAgainCameras(table))
            self.counter += 1
            img = self.same((what, "renderAgainCameras", self.counter))
        return img

    def close(self):
        off = self.off.lookaheadStats()
        for t in (self.on, self.off):
            assert t.walkOverflow() == 0
            t.close()
        assert off[0] == 0 and off[1] == 0 and off[3] == 0      # the comparison context never looked ahead


# ---- 1. the schedule rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("name", ["c2", "all_kinds"])
def test_call_s_looks_through_block_s_mod_n(name, n, arith):
    scene, cam, w, h = _workload(name)
    table = table_of(cam, n, w, h)
    a, b = T(w, h, scene=scene, seed=cases.SEED), T(w, h, scene=scene, seed=cases.SEED)
    try:
        for t in (a, b):
            t.setArith(arith)
            t.setOption(t.OPT_LOOKAHEAD, 0)
        a.render(table[0])
        b.render(table[0])
        for s in range(1, 2 * n + 4):
            a.renderAgainCameras(table)
            b.renderAgain(table[s % n])
            assert a.sample_counter == b.sample_counter == s
            assert np.array_equal(bits(a.transferImage()), bits(b.transferImage())), (name, n, s)
        assert a.lookaheadStats() == (0, 0, 2 * n + 3, 0)
    finally:
        a.close()
        b.close()


# ---- 2. look-ahead equals the direct kernel ------------------------------------------------------------------------------
# (K, n): (5, 3) the table wraps inside a batch; (16, 100) a batch starts across the wrap; (16, 1) one block
KN = [(2, 64), (5, 3), (16, 100), (64, 64), (16, 1)]
SEQUENCES = [("c2", k, n, None) for k, n in KN] + [
    ("all_kinds", 5, 3, None), ("all_kinds", 16, 100, None), ("c3", 2, 64, None), ("c5", 5, 3, None), ("c5", 16, 1, None),
    ("c4", 16, 100, None),
    ("all_kinds", 5, 3, 2)]         # RT_OPT_ACCEL 2: a sphere BVH beside a lens and small meshes, the (1, 1) row
ROW = {("c2", None): (0, 0), ("all_kinds", None): (0, 1), ("c3", None): (0, 1), ("c5", None): (1, 2), ("c4", None): (1, 0),
       ("all_kinds", 2): (1, 1)}


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("name,k,n,accel", SEQUENCES)
def test_sequence_equals_the_direct_kernel(name, k, n, accel, fill, arith):
    scene, cam, w, h = _workload(name)
    table = table_of(cam, n, w, h)
    p = Pair(w, h, scene, arith, k, fill=fill, accel=accel)
    try:
        calls = 2 * k + 3
        p.render(table[0], (name, k, n))
        img = p.cameras(table, (name, k, n, fill, arith), calls)
        assert np.isfinite(img).all() and img[..., :3].sum() > 0 and (img[..., 3] == 1).all()
        # the first call meets a new table and runs direct; every later one is served, a batch per K of them
        assert p.stats() == (-(-(calls - 1) // k), calls - 1, 1, 0), (name, k, n)
        assert p.off.lookaheadStats() == (0, 0, calls, 0)
        facts, plan = p.on.lastCameraPlan()
        assert plan["family"] == QUEUE and facts["count"] == k and facts["moments"] == 0
        assert (plan["accel"], plan["geom"]) == ROW[(name, accel)]
    finally:
        p.close()


# ---- 3. one block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 2])
def test_a_table_of_one_block_is_plain_render_again(arith):
    scene, cam, w, h = _workload("c2")
    a, b = T(w, h, scene=scene, seed=cases.SEED), T(w, h, scene=scene, seed=cases.SEED)
    try:
        for t in (a, b):
            t.setArith(arith)
            t.setOption(t.OPT_LOOKAHEAD, 4)
        a.render(cam)
        b.render(cam)
        for s in range(1, 12):
            a.renderAgainCameras(np.asarray(cam, np.float32).reshape(1, 12))
            b.renderAgain(cam)
            assert np.array_equal(bits(a.transferImage()), bits(b.transferImage())), s
        assert a.lookaheadStats() == (3, 10, 1, 0)      # the table is new to the first call
        assert b.lookaheadStats() == (3, 11, 0, 0)      # the camera block is render's
    finally:
        a.close()
        b.close()


# ---- 4. tiny frames and extreme scenes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("kind", ["1x1", "empty", "all_sky"])
def test_frames_with_next_to_nothing_in_them(kind, arith):
    if kind == "empty":
        scene = rt.SceneCreator()
        scene.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
        cam, w, h = rt.Camera(60, 33 / 17).transferData(), 33, 17
    elif kind == "1x1":
        scene, cam, _, _ = _workload("all_kinds")
        w, h = 1, 1
    else:
        scene = rt.SceneCreator()
        scene.addMaterial(rt._abi.T_DIFFUSE, (0.9, 0.5, 0.2), 1)
        scene.addMaterial(rt._abi.T_LIGHT, (1, 1, 1), 0)
        scene.addSphere((0, 0, -300), 100, 1)
        cam, w, h = rt.Camera(60, 1.0, (0, 0, 0), 0.0, 0.0).transferData(), 128, 128
    table = table_of(cam, 5, w, h)
    p = Pair(w, h, scene, arith, 4)
    try:
        p.render(table[0], kind)
        p.cameras(table, kind, 11)
        assert p.stats() == (3, 10, 1, 0)
    finally:
        p.close()


# ---- 5. drops ----------------------------------------------------------------------------------------------------------------
def _one_bit(table):
    t = table.copy()
    t.view(np.uint32)[len(t) // 2, 4] ^= 1
    return t


@pytest.mark.parametrize("arith", [0, 2])
def test_every_change_drops_the_pending_frames(arith):
    """In the middle of a batch one thing changes at a time, on both contexts.  The next images must equal the comparison
    context's, and the frames computed before the change must have been dropped."""
    wl = rt.workloads.get("all_kinds", width=120, height=72)
    cam, scene, w, h = wl.camera, wl.scene, wl.width, wl.height
    other = rt.workloads.get("c2", width=120, height=72).scene
    table = table_of(cam, 6, w, h)
    p = Pair(w, h, scene, arith, 8)
    try:
        def pending(st):
            """frames computed and neither handed out nor dropped: every batch here has 8 (the counter stays small)"""
            return 8 * st[0] - st[1] - st[3]

        def settle():
            """render + 4 table calls: a batch of 8 has been launched (by the first call if it repeats the remembered table,
            else by the second) and 4 or 5 of its frames are pending"""
            b0 = p.stats()[0]
            p.render(table[0], "settle")
            assert pending(p.stats()) == 0
            p.cameras(table, "settle", 4)
            st = p.stats()
            assert st[0] == b0 + 1 and pending(st) in (4, 5)
            return st

        def after(what, before, direct=False):
            p.cameras(table, what, 3)
            b, s, dr, d = p.stats()
            assert d == before[3] + pending(before), (what, before, (b, s, dr, d))
            if direct:
                assert dr == before[2] + 3 and b == before[0], (what, before, (b, s, dr, d))
            else:
                assert b == before[0] + 1, (what, before, (b, s, dr, d))

        # one bit of the table: that call runs the direct kernel and is remembered, the next one starts a batch
        st = settle()
        changed = _one_bit(table)
        assert pending(st) == 5                       # (the very first table call of the context met no table)
        p.cameras(changed, "one bit")
        assert p.stats() == (st[0], st[1], st[2] + 1, st[3] + 5)
        p.cameras(changed, "one bit", 2)
        assert p.stats() == (st[0] + 1, st[1] + 2, st[2] + 1, st[3] + 5)
        # n_cameras: a prefix of the same table is another table
        st = settle()
        pend = pending(st)
        p.cameras(table[:5], "n_cameras")
        assert p.stats() == (st[0], st[1], st[2] + 1, st[3] + pend)
        p.cameras(table[:5], "n_cameras", 2)
        assert p.stats() == (st[0] + 1, st[1] + 2, st[2] + 1, st[3] + pend)
        # a plain renderAgain in between: direct (it repeats no plain call), and the table call after it repeats no table call
        st = settle()
        pend = pending(st)
        p.renderAgain(table[2], "plain in between")
        assert p.stats() == (st[0], st[1], st[2] + 1, st[3] + pend)
        p.cameras(table, "after the plain call")
        assert p.stats() == (st[0], st[1], st[2] + 2, st[3] + pend)
        p.cameras(table, "after the plain call", 2)
        assert p.stats() == (st[0] + 1, st[1] + 2, st[2] + 2, st[3] + pend)
        # a table call drops a pending PLAIN batch
        p.render(cam, "plain batch")
        p.renderAgain(cam, "plain batch", 3)
        st = p.stats()
        assert pending(st) == 5
        p.cameras(table, "table after a plain batch")
        assert p.stats() == (st[0], st[1], st[2] + 1, st[3] + 5)
        # render
        st = settle()
        p.render(table[0], "render")
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
        # an option
        st = settle()
        p.do(lambda t: t.setOption(t.OPT_ACCEL, 0))
        after("option", st)
        p.do(lambda t: t.setOption(t.OPT_ACCEL, 1))
        # a new scene
        st = settle()
        p.do(lambda t: t.setScene(other))
        p.counter = 0                                 # (rt_set_scene resets the sample counter)
        after("scene", st)
        p.do(lambda t: t.setScene(scene))
        # the seed
        st = settle()
        p.do(lambda t: t.setSeed(12345))
        after("seed", st)
        p.do(lambda t: t.setSeed(cases.SEED))
        settle()
    finally:
        p.close()


# ---- 6. fallbacks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("kind", ["counters", "shard", "no_queue", "split"])
def test_contexts_a_batch_cannot_serve_run_the_direct_kernel(kind, arith):
    scene, cam, w, h = _workload("all_kinds")
    table = table_of(cam, 7, w, h)
    p = Pair(w, h, scene, arith, 8)
    try:
        if kind == "counters":
            def counting(t):
                t.enableCounters(True)
                t.resetCounters()
            p.do(counting)
        elif kind == "shard":
            p.do(lambda t: t.setShard(0, 2, 8, 8))
        elif kind == "no_queue":
            p.do(lambda t: t.setOption(t.OPT_SAMPLE_QUEUE, 0))
        else:
            p.do(lambda t: t.setOption(t.OPT_MAX_THREADS_PER_LAUNCH, 4096))
        p.render(table[0], kind)
        p.cameras(table, kind, 10)
        assert p.stats() == (0, 0, 10, 0)
        if kind == "counters":
            cn = p.on.counters().as_dict()
            assert cn == p.off.counters().as_dict() and cn["samples"] == 11 * w * h
        # prefix sharing does not matter: camera launches share no prefix
        if kind == "no_queue":
            p.do(lambda t: t.setOption(t.OPT_SAMPLE_QUEUE, 1))
            p.do(lambda t: t.setOption(t.OPT_PREFIX_SHARING, 0))
            p.cameras(table, "no prefix sharing", 8)       # (the table is the remembered one: the first call starts the batch)
            assert p.stats() == (1, 8, 10, 0)
    finally:
        p.close()


# ---- 7. nothing else moves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 2])
def test_nothing_else_moves(arith):
    scene, cam, w, h = _workload("all_kinds")
    table = table_of(cam, 5, w, h)
    p = Pair(w, h, scene, arith, 4)
    try:
        def setup(t):
            t.setOption(t.OPT_MOMENTS, 1)
            t.clear()
            t.renderSamples(cam, 0, 8)
            t.renderSamples(cam, 8, 8)          # (the second call reuses the kept prefix: the entry is valid)
            t.renderFeatures(cam)
        p.do(setup)
        acc, m2, feat = p.on.readLinear(), p.on.moments(), p.on.featureRecords()
        cache = p.on.prefixCacheStats()
        assert cache[0] >= 1
        p.render(table[0])
        p.cameras(table, "moments on", 10)
        assert p.stats() == (3, 9, 1, 0)                            # batches did happen, moments or not
        facts, plan = p.on.lastCameraPlan()
        assert plan["family"] == QUEUE and facts["moments"] == 0
        for t in (p.on, p.off):
            assert np.array_equal(bits(t.readLinear()), bits(acc))
            assert np.array_equal(bits(t.moments()), bits(m2))
            assert t.featureRecords().tobytes() == feat.tobytes()
        assert p.on.prefixCacheStats() == cache
        # the kept prefix still serves the fused path
        p.do(lambda t: t.renderSamples(cam, 16, 8))
        assert p.on.prefixCacheStats() == (cache[0] + 1, cache[1])
        assert np.array_equal(bits(p.on.readLinear()), bits(p.off.readLinear()))
        # and the image still continues where it was
        p.cameras(table, "after the fused call", 3)
    finally:
        p.close()


def test_one_history_entry_per_call():
    scene, cam, w, h = _workload("c2")
    table = table_of(cam, 3, w, h)
    t = T(w, h, scene=scene, seed=cases.SEED)
    try:
        t.setOption(t.OPT_LOOKAHEAD, 4)
        t.render(table[0])
        assert len(t.kernelMsHistory()) == 1
        for i in range(10):                      # direct, batch, served, served, served, batch, ...
            t.renderAgainCameras(table)
            assert len(t.kernelMsHistory()) == 2 + i
        assert t.lookaheadStats() == (3, 9, 1, 0)
        first, second = t.stageMsHistory()
        assert len(first) == len(second) == 11 and all(v >= 0 for v in first + second)
        assert all(v > 0 for v in t.kernelMsHistory())
    finally:
        t.close()


def test_error_codes_and_a_failed_call_changes_nothing():
    scene, cam, w, h = _workload("c2")
    table = table_of(cam, 3, w, h)
    t = T(w, h, scene=scene, seed=cases.SEED)
    lib = t._lib
    try:
        t.render(table[0])
        t.renderAgainCameras(table)
        img, st = t.transferImage().copy(), t.lookaheadStats()
        big = np.zeros((4097, 12), np.float32)
        assert lib.rt_render_again_cameras(t._ctx, None, 3) == EINVAL
        assert lib.rt_render_again_cameras(t._ctx, table.ctypes.data, 0) == EINVAL
        assert lib.rt_render_again_cameras(t._ctx, big.ctypes.data, 4097) == EINVAL
        assert lib.rt_render_again_cameras(None, table.ctypes.data, 3) == EINVAL
        assert t.sample_counter == 1 and t.lookaheadStats() == st
        assert np.array_equal(bits(t.transferImage()), bits(img))
        with pytest.raises(ValueError):
            t.renderAgainCameras(np.zeros((4, 11), np.float32))
        t.renderAgainCameras(np.tile(table, (1366, 1))[:4096])        # the largest table
        assert t.sample_counter == 2
    finally:
        t.close()
    ctx = rt.raytracer.C.c_void_p()
    assert lib.rt_create(0, 16, 16, rt.raytracer.C.byref(ctx)) == 0
    try:
        assert lib.rt_render_again_cameras(ctx, table.ctypes.data, 3) == ESTATE       # no scene
    finally:
        lib.rt_destroy(ctx)


# ---- 8. rt_cli -----------------------------------------------------------------------------------------------------------------
def test_cli_progressive_cameras_writes_the_same_file_and_the_python_image(built, tmp_path):
    cli = os.path.join(cases.ROOT, "host", "rt_cli")
    path = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")      # (no textures: the two hosts' scenes are the same bits)
    w, h, spp = 64, 40, 20
    out = {}
    for k in (8, 0):
        raw = str(tmp_path / ("k%d.f32" % k))
        subprocess.run([cli, "--scene", path, "--size", "%dx%d" % (w, h), "--spp", str(spp), "--camera=-8,-1,-8,45,0", "--aa",
                        "--progressive-cameras", "--lookahead", str(k), "--raw", raw], check=True, cwd=cases.ROOT)
        out[k] = np.fromfile(raw, np.float32).reshape(h, w, 4)
    assert np.array_equal(bits(out[8]), bits(out[0]))
    scene = rt.SceneCreator()
    scene.loadScene(path, base_dir=os.path.join(cases.ROOT, "assets"))
    table = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0).sampleBlocks(spp, width=w, height=h)
    t = T(w, h, scene=scene, seed=cases.SEED)
    try:
        t.setOption(t.OPT_LOOKAHEAD, 8)
        t.render(table[0])
        for _ in range(spp - 1):
            t.renderAgainCameras(table)
        assert np.array_equal(bits(t.transferImage()), bits(out[8]))
        assert t.lookaheadStats()[0] == 3
    finally:
        t.close()
