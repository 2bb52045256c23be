"""GPU (-m gpu): a cleared frame is stored, not added to (RT_OPT_ACCUM_STORE, include/rt_amd.h; csrc/pt_sample.hpp
accumulate_store, csrc/pt_kernels.hip launch_fused_any).  Under RT_OPT_ACCUM_STORE 1 rt_clear records the clear, a qualifying fused
launch stores 0 + sum over whatever the frame held, and everything else enqueues the memset first.  Every result here is
compared word for word (uint32, ==) with the SAME library under RT_OPT_ACCUM_STORE 0, where rt_clear enqueues the memset at
once and every launch adds — the parent's behaviour.

The accumulator is read through ONE torch view of the rt_device_accum pointer, taken when the tracer is made — before any
clear — and read after sync(): the path distributed.GpuShard uses, and the one on which a clear that was recorded and never
enqueued would show (the view would still hold the frame before the clear).  Every sequence starts on a DIRTY accumulator:
a frame rendered before the first clear, so that a store arm that added, or a memset that never came, changes words.
rt_accum_store_stats says how each recorded clear ended, so a run in which no launch ever stored cannot pass.

(a) C2 and C3 at 61 x 37 and 7 x 5 — no multiple of the six pixels a wave owns — and C2 from inside its glass sphere, at
    1, 5, 24, 64, 100 and 512 samples (both sides of the COUNT_LOG2 = 6 kernel and of PT_TREE_MIN_SAMPLES), every policy:
    first after a traced prefix (pt_prefix stores the finished pixels), then again with the prefix kept (pt_final_replay
    does) — at 64 samples, the one count whose launches store; every other count takes the memset and the generic-count
    kernel's add, as before.  w included.  The reference run lights more than 0.2 of every frame from 5 samples a pixel on
    and more than 0.38 / 4 at one sample.
(b) Sequences around the clear, each non-qualifying consumer among them.
(c) lastSamplePlan() does not depend on the mode."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
T = rt.RayTracer
f32 = np.float32
POLICIES = [0, 1, 2]
COUNTS = (1, 5, 24, 64, 100, 512)
SIZES = {"ragged": (61, 37), "tiny": (7, 5)}
GLASS_CENTRE = (0.0, 3.2, -0.5)   # C2's refractive sphere, r = 1.8 (assets/scenes/c2_cornell.scene)
FRAMES = [("c2", "ragged"), ("c2", "tiny"), ("c3", "ragged"), ("c3", "tiny"), ("c2_inside_glass", "ragged")]
GEOM = {"c2": 0, "c3": 1, "c2_inside_glass": 0}


def _workload(case, size):
    w, h = SIZES[size]
    if case == "c3":
        return rt.workloads.get("c3", width=w, height=h, tex_size=64)
    wl = rt.workloads.get("c2", width=w, height=h)
    if case == "c2_inside_glass":
        assert int(wl.scene.materials["type"][wl.scene.spheres["mat_ID"][2]]) == A.T_REFRACTIVE
        assert tuple(wl.scene.spheres["pos"][2][:3]) == GLASS_CENTRE
        wl.camera = rt.Camera(60, f32(w) / f32(h), GLASS_CENTRE, 45.0, 0.0).transferData()
    return wl


class Rig:
    """A tracer and the view of its accumulator taken before any clear."""

    def __init__(self, wl, policy):
        import torch
        self.wl = wl
        self.t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
        self.t.setArith(policy)
        self.acc = torch.as_tensor(self.t.deviceAccum(), device="cuda")
        assert tuple(self.acc.shape) == (wl.height, wl.width, 4)

    def read(self):
        """The accumulator's words through the old view, after sync()."""
        self.t.sync()
        return self.acc.cpu().numpy().copy().view(np.uint32)

    def dirty(self, spp=3, first=11):
        """Leaves a frame of other samples in the accumulator (added to whatever it holds), and no kept prefix (every
        setOption drops it): the next fused call traces its prefix."""
        self.t.renderSamples(self.wl.camera, first, spp)
        self.t.setOption(T.OPT_PREFIX_CACHE, 1)

    def close(self):
        self.t.close()


def _modes(rig, sequence):
    """sequence(rig) under RT_OPT_ACCUM_STORE 1, then 0, each from a dirty accumulator → ([what it returned], stats of the
    store mode's run: (stored, materialised) clears)."""
    out, stats = [], None
    for mode in (1, 0):
        rig.t.setOption(T.OPT_ACCUM_STORE, mode)
        rig.dirty()
        before = rig.t.accumStoreStats()
        out.append(sequence(rig))
        after = rig.t.accumStoreStats()
        delta = (after[0] - before[0], after[1] - before[1])
        if mode:
            stats = delta
        else:
            assert delta == (0, 0), delta   # (nothing is recorded under 0)
    rig.t.setOption(T.OPT_ACCUM_STORE, 1)
    return out, stats


def _same(got, ref, what):
    got, ref = (x if isinstance(x, (list, tuple)) else [x] for x in (got, ref))
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype == np.uint32, (what, k)
        bad = g != r
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist(), g[bad][:4], r[bad][:4])


# ---- (a) accumulators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("case,size", FRAMES)
def test_stored_frames_equal_added_frames(case, size, policy):
    wl = _workload(case, size)
    rig = Rig(wl, policy)
    t = rig.t
    try:
        for spp in COUNTS:
            def sequence(rig):
                misses = t.prefixCacheStats()[1]
                t.clear()
                t.renderSamples(wl.camera, 0, spp)     # (no kept prefix: pt_prefix runs)
                assert t.prefixCacheStats()[1] == misses + 1
                traced = rig.read()
                facts, plan = t.lastSamplePlan()
                assert plan["family"] == A.PLAN_QUEUE and plan["accel"] == 0 and plan["geom"] == GEOM[case], (case, spp, plan)
                assert facts["count_enabled"] == 0 and facts["moments"] == 0, facts
                assert (plan["count_log2"] == 6) == (spp == 64), (spp, plan)
                hits = t.prefixCacheStats()[0]
                t.clear()
                t.renderSamples(wl.camera, 0, spp)     # (the prefix is kept: pt_final_replay runs)
                assert t.prefixCacheStats()[0] == hits + 1
                return [traced, rig.read()]
            (got, ref), stats = _modes(rig, sequence)
            # at 64 samples both clears ended in a storing launch; the generic-count kernels keep the add, behind the memset
            assert stats == ((2, 0) if spp == 64 else (0, 2)), (case, size, policy, spp, stats)
            _same(got, ref, (case, size, policy, spp))
            _same(ref[0], ref[1], "a replayed prefix gives the traced one's bits")
            frame = ref[0].view(f32)
            assert (frame[..., 3] == f32(spp)).all(), (case, size, policy, spp)
            lit = float((frame[..., :3] > 0).any(axis=2).mean())
            print("%s %s policy %d, %d spp: %.3f of the pixels are lit" % (case, size, policy, spp, lit))
            # A black frame would pass whatever the code does.  More than 0.2 of every frame is lit, as the CPU oracle has it
            # (0.38 .. 0.54 with 4 samples a pixel, profiles/r30_experiments.md §7), at every count from 5 on — the storing
            # count, 64, among them.  ONE sample lights a pixel only if that one path ends on the light; a frame of which four
            # samples light 0.38 is lit by one of them to 0.38 / 4 at the least (the union of four is at most their sum).
            assert lit > (0.2 if spp >= 5 else 0.38 / 4), (case, size, policy, spp, lit)
    finally:
        rig.close()


# ---- (b) sequences -------------------------------------------------------------------------------------------------------------
def _rig(policy=2, case="c2", size="ragged"):
    return Rig(_workload(case, size), policy)


def _check(sequence, stats, policy=2, case="c2"):
    rig = _rig(policy, case)
    try:
        (got, ref), st = _modes(rig, sequence)
        assert st == stats, (st, stats)
        _same(got, ref, sequence.__name__)
        return ref
    finally:
        rig.close()


def test_the_second_render_adds():
    def clear_render_render(rig):
        t, cam = rig.t, rig.wl.camera
        t.clear()
        t.renderSamples(cam, 0, 64)
        t.renderSamples(cam, 64, 24)
        return rig.read()
    ref = _check(clear_render_render, (1, 0))
    assert (ref.view(f32)[..., 3] == 88).all()


def test_a_call_of_several_launches_adds_to_the_cleared_frame():
    def clear_render_1100(rig):   # 512 + 512 + 76: no launch of 64, the clear is the memset in front of the first
        rig.t.clear()
        rig.t.renderSamples(rig.wl.camera, 0, 1100)
        return rig.read()
    ref = _check(clear_render_1100, (0, 1), case="c2")
    assert (ref.view(f32)[..., 3] == 1100).all()


def test_clear_clear_render():
    def clear_clear_render(rig):
        rig.t.clear()
        rig.t.clear()
        rig.t.renderSamples(rig.wl.camera, 0, 64)
        return rig.read()
    _check(clear_clear_render, (1, 1))   # (the first clear is enqueued before the second is recorded)


def test_clear_then_read():
    def clear_read_linear(rig):
        rig.t.clear()
        lin = rig.t.readLinear()
        assert not lin.view(np.uint32)[..., :3].any()
        return [np.ascontiguousarray(lin).view(np.uint32), rig.read()]
    ref = _check(clear_read_linear, (0, 1))
    assert not ref[1].any()

    def clear_sync(rig):   # nothing but the wait for the stream stands between the clear and the caller's view
        rig.t.clear()
        return rig.read()
    ref = _check(clear_sync, (0, 1))
    assert not ref.any()


def test_clear_then_resolve():
    def clear_resolve(rig):
        rig.t.clear()
        rig.t.resolve()
        image = np.ascontiguousarray(rig.t.transferImage()).view(np.uint32)
        return [image, rig.read()]
    _check(clear_resolve, (0, 1))


def test_render_64_clear_render_24():
    def r64_clear_r24(rig):
        t, cam = rig.t, rig.wl.camera
        t.clear()
        t.renderSamples(cam, 0, 64)
        first = rig.read()
        t.clear()
        t.renderSamples(cam, 0, 24)
        return [first, rig.read()]
    ref = _check(r64_clear_r24, (1, 1))
    assert (ref[1].view(f32)[..., 3] == 24).all()


def test_clear_set_scene_render():
    other = _workload("c3", "ragged")

    def clear_scene_render(rig):
        rig.t.clear()
        rig.t.setScene(other.scene)
        rig.t.renderSamples(other.camera, 0, 64)
        out = rig.read()
        rig.t.setScene(rig.wl.scene)
        return out
    _check(clear_scene_render, (0, 1))   # (rt_set_scene waits for the stream)


@pytest.mark.parametrize("policy", POLICIES)
def test_clear_then_a_consumer_that_does_not_qualify(policy):
    """Each of these enqueues the memset and runs as ever: a masked adaptive round, rays into the accumulator, the camera
    table, packAccum on rank 0 of 2, moments on, counters on."""
    import torch
    rig = _rig(policy)
    t, wl = rig.t, rig.wl
    w, h = wl.width, wl.height
    try:
        t.renderFeatures(wl.camera)
        rec = t.featureRecords()
        ys, xs = np.mgrid[0:h, 0:w]
        batch = rt.rays.pack_rays(np.asarray(wl.camera, f32)[0:3], rec["dir"].reshape(-1, 3),
                                  ids=np.stack([xs.ravel(), ys.ravel()], axis=1))
        t.uploadRays(batch)
        blocks = np.tile(np.asarray(wl.camera, f32).reshape(1, 12), (24, 1))

        def adaptive(rig):   # (later rounds trace the blocks still active: masked launches)
            t.clear()
            st = t.renderAdaptive(wl.camera, 0.02, batch=8, min_spp=16, max_spp=48)
            assert st["rounds"] >= 2, st
            return rig.read()

        def rays(rig):
            t.clear()
            t.renderRays(None, 0, 24)
            return rig.read()

        def camera_table(rig):
            t.clear()
            t.renderSamplesCameras(blocks, 0)
            return rig.read()

        def pack(rig):
            t.setShard(0, 2, 8, 8)
            t.clear()
            n = t.shardSlots(2)
            packed = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            t.packAccum(packed.data_ptr(), n * 16)
            out = [rig.read(), packed.cpu().numpy().view(np.uint32)]
            t.renderSamples(wl.camera, 0, 24)   # (a sharded frame never qualifies)
            out.append(rig.read())
            t.setShard(0, 1, 8, 8)
            return out

        def moments(rig):
            t.setOption(T.OPT_MOMENTS, 1)
            t.clear()
            t.renderSamples(wl.camera, 0, 24)
            out = [rig.read(), np.ascontiguousarray(t.moments()).view(np.uint32)]
            t.setOption(T.OPT_MOMENTS, 0)
            return out

        def counters(rig):
            t.enableCounters(True)
            t.clear()
            t.renderSamples(wl.camera, 0, 24)
            out = rig.read()
            t.enableCounters(False)
            return out

        for sequence, stats in ((adaptive, (0, 0)), (rays, (0, 1)), (camera_table, (0, 1)), (pack, (0, 1)), (moments, (0, 1)),
                                (counters, (0, 1))):
            (got, ref), st = _modes(rig, sequence)
            assert st == stats, (sequence.__name__, st)   # (adaptive: the call's own memset IS the pending clear)
            _same(got, ref, (policy, sequence.__name__))
            last = (ref[-1] if isinstance(ref, list) else ref).view(f32)
            assert (last[..., :3] > 0).any(), sequence.__name__
    finally:
        rig.close()


# ---- (c) the plan --------------------------------------------------------------------------------------------------------------
def test_the_sample_plan_does_not_depend_on_the_mode():
    rig = _rig(2)
    try:
        for spp in (5, 64, 100):
            def plan_of(rig):
                rig.t.clear()
                rig.t.renderSamples(rig.wl.camera, 0, spp)
                rig.t.sync()
                return rig.t.lastSamplePlan()
            plans = []
            for mode in (1, 0):
                rig.t.setOption(T.OPT_ACCUM_STORE, mode)
                plans.append(plan_of(rig))
                plans.append(plan_of(rig))   # (with the prefix kept: the exact grid)
            assert plans[0] == plans[2] and plans[1] == plans[3], (spp, plans)
    finally:
        rig.close()
