"""GPU (-m gpu): ray sets (rt_render_ray_sets) — a set of records per ray, sample s of ray i starting at record s mod
set_size of the ray's set.  Sets built from the primary rays of camera blocks — their bits taken from the library itself:
renderFeatures(block)'s `dir` per pixel under the selected policy, the origin block[0:3] — must give
rt_render_spp_cameras' accumulator bit for bit in every row of the queue family and in the fixed-lane family; a sample
must be rt_render_rays' sample of its own record; the cyclic rule, the launch cut, the accumulator target, the moments, the
state rules and the errors are pinned beside them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import moments_ref as M
import denoise_vg_ref as V

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
R = rt.raytracer
T = rt.RayTracer
rays_mod = rt.rays
EINVAL, ESTATE = -1, -4
FIXED, QUEUE = A.CAMERA_PLAN_FIXED, A.CAMERA_PLAN_QUEUE
W, H = 48, 27
POLICIES = [0, 1, 2]
CAMERA = rt.Camera(60, np.float32(W) / np.float32(H), (-8, -1, -8), 45.0, 0.0)


def blocks_for(n, w=W, h=H, camera=CAMERA):
    return camera.sampleBlocks(n, width=w, height=h, aperture=0.05, focus=8)


def tracer(wl, policy=0, **options):
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    if policy:
        t.setArith(policy)
    for k, v in options.items():
        t.setOption(getattr(T, k), v)
    return t


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def primary_batch(t, camera):
    """The block's primary rays with the selected policy's own direction bits, ids = pixel coordinates → RAY (h * w,)."""
    t.renderFeatures(camera)
    rec = t.featureRecords()
    h, w = rec.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return rays_mod.pack_rays(np.asarray(camera, np.float32)[0:3], rec["dir"].reshape(-1, 3),
                              ids=np.stack([xs.ravel(), ys.ravel()], axis=1))


def block_sets(t, blocks):
    """(w * h, len(blocks)) RAY: record (i, j) = pixel i's primary ray through block j"""
    return np.stack([primary_batch(t, b) for b in blocks], axis=1)


def to_device(records):
    import torch
    return torch.from_numpy(rays_mod.as_floats(np.ascontiguousarray(records).reshape(-1)).copy()).cuda()


def render_sets(t, sets, first, n, flat=True):
    """renderRaySets of host sets (n_rays, k) as a torch tensor into a zeroed external buffer → (n_rays, 4) float32"""
    import torch
    n_rays, k = sets.shape
    d = to_device(sets)
    if not flat:
        d = d.reshape(n_rays, k, 8)
    out = torch.zeros((n_rays, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t.renderRaySets(d, k, first, n, out=out)
    t.sync()
    return out.cpu().numpy()


def render_batch(t, batch, first, n):
    import torch
    d = to_device(batch)
    out = torch.zeros((len(batch), 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t.renderRays(d, first, n, out=out)
    t.sync()
    return out.cpu().numpy()


def cameras_accum(t, blocks, first=0):
    t.clear()
    t.renderSamplesCameras(blocks, first)
    return read_accum(t).reshape(-1, 4)


# ---- 1. camera parity, all five queue rows, every policy -------------------------------------------------------------------
SCENES = {   # workload, its arguments at 48 x 27 → the (ACCEL, GEOM) row of the queue its launches must run
    "c2": (dict(), (0, 0)),
    "all_kinds": (dict(), (0, 1)),
    "c3": (dict(tex_size=64), (0, 1)),
    "c4": (dict(n_spheres=3000), (1, 0)),
    "c5": (dict(segments=24, rings=16), (1, 2)),
}


def workload(name):
    kw, row = SCENES[name]
    return rt.workloads.get(name, width=W, height=H, **kw), row


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_camera_parity_in_every_queue_row(name, policy):
    wl, row = workload(name)
    counts = (1, 5, 64, 512) if name == "c2" else (1, 5, 64)
    blocks = blocks_for(max(counts))                 # (the blocks of n samples are the first n of these)
    t = tracer(wl, policy)
    try:
        sets = block_sets(t, blocks)
        for n in counts:
            want = cameras_accum(t, blocks[:n])
            got = render_sets(t, np.ascontiguousarray(sets[:, :n]), 0, n, flat=n != 5)
            facts, plan = t.lastRayPlan()
            assert (plan["family"], plan["accel"], plan["geom"]) == (QUEUE,) + row, (name, n, plan)
            assert plan == R.plan_camera_samples(**facts) and facts["n"] == W * H and facts["count"] == n
            assert (want[:, 3] == n).all() and want[:, :3].any()
            assert same_bits(got, want), (name, policy, n)
            t.clear()
            t.renderSamples(CAMERA.transferData(), 0, n)
            assert not same_bits(read_accum(t).reshape(-1, 4), want), "the jitter and the lens move the frame"
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 2. the cyclic rule, the stride, the launch cut --------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_cyclic_rule_stride_and_launch_cut(policy):
    wl, _ = workload("c2")
    blocks = blocks_for(16)
    t = tracer(wl, policy)
    try:
        sets = block_sets(t, blocks)
        five = np.ascontiguousarray(sets[:, :5])
        want = cameras_accum(t, blocks[[(7 + j) % 5 for j in range(24)]], 7)
        assert same_bits(render_sets(t, five, 7, 24), want)
        assert not same_bits(cameras_accum(t, blocks[[j % 5 for j in range(24)]], 7), want)   # (the rule says something)
        eight = np.ascontiguousarray(sets[:, :8])        # a prefix of each set is read: the stride is not the count
        assert same_bits(render_sets(t, eight, 0, 3), cameras_accum(t, blocks[:3], 0))
        want = cameras_accum(t, blocks[[j % 16 for j in range(520)]], 0)
        got = render_sets(t, sets, 0, 520)
        facts, _ = t.lastRayPlan()
        assert facts["count"] == 8 and (want[:, 3] == 520).all() and same_bits(got, want)
    finally:
        t.close()


# ---- 3. degenerate sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_degenerate_sets_are_render_rays(policy):
    wl, _ = workload("c2")
    t = tracer(wl, policy)
    try:
        batch = primary_batch(t, wl.camera)
        for first, n in ((0, 24), (5, 1)):
            want = render_batch(t, batch, first, n)
            assert want[:, :3].any()
            assert same_bits(render_sets(t, batch.reshape(-1, 1), first, n), want)
            assert same_bits(render_sets(t, np.repeat(batch.reshape(-1, 1), 6, axis=1), first, n), want)
    finally:
        t.close()


# ---- 4. per-sample decomposition, slot independence --------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_per_sample_decomposition_and_slot_independence(policy):
    wl, _ = workload("c2")
    k = 5
    t = tracer(wl, policy)
    try:
        sets = block_sets(t, blocks_for(k))
        # records of one set with ids of their own: record t of ray (x, y) draws from the stream (x + 3 t, y + t)
        own = sets.copy()
        own["x"] = (own["x"] + 3 * np.arange(k, dtype=np.uint32)[None, :]) % W
        own["y"] = (own["y"] + np.arange(k, dtype=np.uint32)[None, :]) % H
        for s in (0, 3, 7, 65535):
            want = render_batch(t, np.ascontiguousarray(sets[:, s % k]), s, 1)
            assert (want[:, 3] == 1).all() and same_bits(render_sets(t, sets, s, 1), want), s
            mine = render_sets(t, own, s, 1)
            assert same_bits(mine, render_batch(t, np.ascontiguousarray(own[:, s % k]), s, 1)), s
            if s % k:
                assert not same_bits(mine, want), "a record's own ids are used"
        n = 16
        cut = 3 * W * H - 5                                 # not a multiple of any wave's pixels
        full = np.concatenate([sets, own, sets[::-1]])[:cut]
        got = render_sets(t, full, 2, n)
        assert same_bits(got[:W * H], render_sets(t, sets, 2, n)) and got[:, :3].any() and (got[:, 3] == n).all()
        perm = np.random.RandomState(5).permutation(cut)
        assert same_bits(render_sets(t, full[perm], 2, n), got[perm])
        for m in (1, 65):
            pick = perm[:m]
            assert same_bits(render_sets(t, full[pick], 2, n), got[pick]), m
    finally:
        t.close()


# ---- 5. the fixed-lane family -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["c2", "c5"])
def test_fixed_lane_family(name, policy):
    wl, _ = workload(name)
    n = 24
    blocks = blocks_for(n)
    t = tracer(wl, policy)
    try:
        sets = block_sets(t, blocks)
        want = cameras_accum(t, blocks)
        t.setOption(T.OPT_SAMPLE_QUEUE, 0)
        got = render_sets(t, sets, 0, n)
        assert t.lastRayPlan()[1]["family"] == FIXED and same_bits(got, want)
        t.setOption(T.OPT_SAMPLE_QUEUE, 1)
        t.enableCounters(True)
        t.resetCounters()
        got = render_sets(t, sets, 0, n)
        mine = t.counters().as_dict()
        _, plan = t.lastRayPlan()
        assert plan["family"] == FIXED and plan["count"] == 1 and same_bits(got, want)
        t.resetCounters()
        assert same_bits(cameras_accum(t, blocks), want)
        theirs = t.counters().as_dict()
        assert mine == theirs and mine["samples"] == W * H * n and mine["bounces"] > 0
    finally:
        t.close()


OPTIONS = {   # honoured exactly as by rt_render_rays: none changes a bit
    "three_slot_ranges": dict(OPT_MAX_THREADS_PER_LAUNCH=W * H * 32 // 3 + 64),       # (24 samples: 32 lanes per ray)
    "three_slot_ranges_fixed_lanes": dict(OPT_MAX_THREADS_PER_LAUNCH=W * H * 32 // 3 + 64, OPT_SAMPLE_QUEUE=0),
    "wave_fill_0": dict(OPT_WAVE_FILL=0),
    "wave_fill_1": dict(OPT_WAVE_FILL=1),
    "no_accel": dict(OPT_ACCEL=0),
}


@pytest.mark.parametrize("name", ["c2", "c5"])
def test_options_change_no_bit(name):
    wl, _ = workload(name)
    n = 24
    blocks = blocks_for(8)
    t = tracer(wl, 2)
    try:
        sets = block_sets(t, blocks)
        want = render_sets(t, sets, 3, n)
        assert same_bits(want, cameras_accum(t, blocks[[(3 + j) % 8 for j in range(n)]], 3))
        t.close()
        for what, options in OPTIONS.items():
            t = tracer(wl, 2, **options)
            assert same_bits(render_sets(t, sets, 3, n), want), what
            facts, plan = t.lastRayPlan()
            if "OPT_MAX_THREADS_PER_LAUNCH" in options:
                assert facts["n"] < W * H, "the last of several slot ranges"
            assert plan["family"] == (FIXED if "OPT_SAMPLE_QUEUE" in options else QUEUE)
            t.close()
    finally:
        t.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_moments_follow_the_camera_call(policy):
    w, h, n = 24, 16, 24
    wl = rt.workloads.get("c2", width=w, height=h)
    cam = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0)
    blocks = blocks_for(n, w, h, cam)
    t = tracer(wl, policy)
    try:
        sets = block_sets(t, blocks)
        ys, xs = np.mgrid[0:h, 0:w]
        s = np.stack([t.traceSamples(blocks[j], xs.reshape(-1), ys.reshape(-1), np.full(w * h, j)) for j in range(n)], axis=1)
        lum = (s.astype(np.float64) @ V.LUM).reshape(h, w, n)
        truth = ((lum - lum.mean(-1, keepdims=True)) ** 2).sum(-1)
        tol = M.tolerance(truth, np.full((h, w), n), lum.max(-1))
        t.uploadRays(sets)
        got = []
        for on in (0, 1):
            t.setOption(T.OPT_MOMENTS, on)
            t.clear()
            t.renderRaySets(None, n, 0, n)
            t.resolve()
            got.append((read_accum(t), t.transferImage()))
            if on:
                assert t.lastRayPlan()[1]["family"] == FIXED and t.lastRayPlan()[1]["moments"] == 1
        assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])     # the option moves no bit
        mine = t.moments()
        assert same_bits(cameras_accum(t, blocks).reshape(got[1][0].shape), got[1][0])
        theirs = t.moments()
        for m2, what in ((mine, "ray sets"), (theirs, "cameras")):
            err = np.abs(m2.astype(np.float64) - truth)
            print("%s: max |M2 - truth| %.3g (largest tolerance %.3g, max M2 %.4g)" % (what, err.max(), tol.max(), truth.max()))
            assert (err <= tol).all() and (m2 >= 0).all(), what
        assert (np.abs(mine.astype(np.float64) - theirs) <= tol).all() and truth.max() > 0
    finally:
        t.close()


# ---- 6. the accumulator as the target -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_accumulator_target_resolve_and_denoise(policy):
    wl, _ = workload("c2")
    k = 64
    blocks = blocks_for(k)
    t = tracer(wl, policy)
    try:
        sets = block_sets(t, blocks)
        central = to_device(primary_batch(t, wl.camera))
        t.clear()
        t.renderSamplesCameras(blocks[:32], 0)
        one = read_accum(t)
        t.renderSamplesCameras(blocks[32:], 32)
        t.resolve()
        two, image = read_accum(t), t.transferImage()
        assert t.uploadRays(sets) == W * H * k
        t.clear()
        t.renderRaySets(None, k, 0, 32)
        assert same_bits(read_accum(t), one)
        t.renderRaySets(None, k, 32, 32)
        t.resolve()
        assert same_bits(read_accum(t), two) and same_bits(t.transferImage(), image)
        assert (t.sampleCounts() == 64).all()
        t.renderFeaturesRays(central)               # the guides of the central, unjittered rays
        img = t.denoise()
        assert np.isfinite(img).all() and img[..., :3].any()
    finally:
        t.close()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing():
    import torch
    wl, _ = workload("c2")
    t = tracer(wl)
    lib = R.load_library()
    try:
        k = 4
        sets = np.repeat(primary_batch(t, wl.camera).reshape(-1, 1), k, axis=1)
        n = len(sets)
        d = to_device(sets)
        out = torch.full((n, 4), 3.0, dtype=torch.float32, device="cuda")
        t.clear()
        t.renderSamples(wl.camera, 0, 4)
        before = read_accum(t)
        torch.cuda.synchronize()
        dp, op = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
        call = lib.rt_render_ray_sets
        assert call(None, dp, n, k, 0, 4, op) == EINVAL
        assert call(t._ctx, dp, 0, k, 0, 4, op) == EINVAL                        # no rays
        assert call(t._ctx, dp, (1 << 28) + 1, 1, 0, 4, op) == EINVAL            # too many
        assert call(t._ctx, dp, n, 0, 0, 4, op) == EINVAL                        # an empty set
        assert call(t._ctx, dp, n, A.RAY_SET_MAX + 1, 0, 4, op) == EINVAL        # too large a set
        assert call(t._ctx, dp, (1 << 19) + 1, 4096, 0, 4, op) == EINVAL         # more than 2^31 records
        assert call(t._ctx, dp, n, k, 65533, 4, op) == EINVAL                    # sample 65536
        assert call(t._ctx, C.c_void_p(d.data_ptr() + 8), n, k, 0, 4, op) == EINVAL   # not 16-byte aligned
        assert call(t._ctx, None, n, k, 0, 4, op) == EINVAL                      # nothing uploaded
        assert call(t._ctx, dp, n - 1, k, 0, 4, None) == EINVAL                  # the accumulator wants W * H rays
        t.uploadRays(sets.reshape(-1)[:n * k - 1])
        assert call(t._ctx, None, n, k, 0, 4, op) == EINVAL                      # fewer records uploaded than n * k
        t.setShard(0, 2, 8, 8)
        assert call(t._ctx, dp, n, k, 0, 4, op) == EINVAL                        # a sharded context
        t.setShard(0, 1, 8, 8)
        with pytest.raises(ValueError):
            t.renderRaySets(d, 0, 0, 1)
        with pytest.raises(ValueError):
            t.renderRaySets(d, A.RAY_SET_MAX + 1, 0, 1)
        with pytest.raises(ValueError):
            t.renderRaySets(d, 7, 0, 1)                                          # not whole sets of 7
        with pytest.raises(ValueError):
            t.renderRaySets(d[:, :6], k, 0, 1)
        with pytest.raises(ValueError):
            t.renderRaySets(d.cpu(), k, 0, 1)
        with pytest.raises(ValueError):
            t.renderRaySets(d.reshape(n, k, 8), 2, 0, 1)                         # (n, k, 8) with another set size
        with pytest.raises(ValueError):
            t.renderRaySets(d, k, 0, 1, out=out[:-1])
        with pytest.raises(ValueError):
            t.renderRaySets(None, 7, 0, 1)                                       # the uploaded records are no sets of 7
        f, p = A.CameraFacts(), A.CameraPlan()
        assert lib.rt_debug_last_ray_plan(t._ctx, C.byref(f), C.byref(p)) == EINVAL   # no ray launch yet: every call failed
        assert same_bits(read_accum(t), before) and (out.cpu().numpy() == 3.0).all()
        assert call(t._ctx, dp, n, k, 65532, 4, op) == 0                         # sample 65535 is the last
        assert call(t._ctx, dp, n, k, 0, 0, op) == 0                             # nothing to do
        t.sync()
        got = out.cpu().numpy()
        assert (got[:, 3] == 7.0).all() and same_bits(read_accum(t), before)
        ctx = C.c_void_p()
        assert lib.rt_create(0, W, H, C.byref(ctx)) == 0
        assert call(ctx, dp, n, k, 0, 4, op) == ESTATE                           # no scene
        lib.rt_destroy(ctx)
    finally:
        t.close()


# ---- 8. the other state ---------------------------------------------------------------------------------------------------------
def test_a_ray_set_call_leaves_the_other_state_alone():
    wl, _ = workload("c2")

    def sequence(with_sets):
        t = tracer(wl)
        sets = block_sets(t, blocks_for(4))
        t.renderFeatures(wl.camera)
        images = []
        t.clear()
        t.renderSamples(wl.camera, 0, 16)           # leaves a kept prefix
        t.render(wl.camera)
        t.renderAgain(wl.camera)
        t.renderAgain(wl.camera)                    # the second call at rest: a look-ahead batch is pending
        images.append(t.transferImage())
        if with_sets:
            assert render_sets(t, sets, 0, 8)[:, 3].min() == 8
            assert same_bits(t.transferImage(), images[-1])
        for _ in range(2):
            t.renderAgain(wl.camera)
            images.append(t.transferImage())
        t.renderSamples(wl.camera, 16, 16)          # hits the kept prefix
        state = (t.lookaheadStats(), t.sample_counter, t.prefixCacheStats(), t.featureRecords().tobytes(), read_accum(t).tobytes())
        t.close()
        return images, state
    a, sa = sequence(False)
    b, sb = sequence(True)
    assert sa == sb and sa[0][1] > 0 and sa[2][0] >= 1       # frames were served from the batch, the prefix was reused
    for x, y in zip(a, b):
        assert same_bits(x, y)


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_ray_sets_match_the_python_path(built, tmp_path):
    w, h, spp, k = 64, 40, 8, 8
    scene = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    raw, raw_dn = str(tmp_path / "f.f32"), str(tmp_path / "d.f32")
    cli = os.path.join(cases.ROOT, "host", "rt_cli")
    common = [cli, "--scene", scene, "--size", "%dx%d" % (w, h), "--spp", str(spp), "--camera=-8,-1,-8,45,0"]
    base = common + ["--projection", "ortho", "--extent", "12"]
    out = subprocess.run(base + ["--ray-sets", str(k), "--raw", raw], check=True, cwd=cases.ROOT, capture_output=True, text=True).stdout
    assert "ray sets" in out
    out = subprocess.run(base + ["--ray-sets", str(k), "--raw", raw_dn, "--denoise"], check=True, cwd=cases.ROOT, capture_output=True,
                         text=True).stdout
    assert "ray sets" in out and "denoised" in out
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    got_dn = np.fromfile(raw_dn, np.float32).reshape(h, w, 4)
    s = rt.SceneCreator()
    s.loadScene(scene, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        kw = dict(pos=(-8, -1, -8), w=w, h=h, extent=12.0, yaw=45.0, pitch=0.0)
        sets = rays_mod.ray_sets(rays_mod.orthographic_rays, rt.Camera.sampleOffsets(k), **kw)
        t.clear()
        t.renderRaySets(sets, k, 0, spp)
        t.resolve()
        exp = t.transferImage()
        t.clear()
        t.renderRays(rays_mod.orthographic_rays(**kw), 0, spp)
        t.resolve()
        assert not same_bits(t.transferImage(), exp), "the jitter moves the frame"
    finally:
        t.close()
    # Both hosts do the arithmetic in double and round once: a record differs between them only where a double lies within
    # an ulp of a float32 rounding boundary, and a pixel only through its records
    assert np.isfinite(got).all() and got[..., :3].any()
    assert (got.view(np.uint32) == exp.view(np.uint32)).all(-1).mean() >= 0.99
    assert np.isfinite(got_dn).all() and got_dn[..., :3].any()
    # the usage rules: ray sets belong to a projection, and --aa stays the pinhole camera's
    assert subprocess.run(common + ["--ray-sets", str(k)], cwd=cases.ROOT, capture_output=True).returncode == 2
    assert subprocess.run(base + ["--ray-sets", "0"], cwd=cases.ROOT, capture_output=True).returncode == 2
    assert subprocess.run(base + ["--ray-sets", str(A.RAY_SET_MAX + 1)], cwd=cases.ROOT, capture_output=True).returncode == 2
    assert subprocess.run(base + ["--aa"], cwd=cases.ROOT, capture_output=True).returncode == 2
