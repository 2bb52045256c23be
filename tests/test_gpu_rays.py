"""GPU (-m gpu): caller-supplied rays (rt_render_rays, rt_render_features_rays).  A batch of a camera's own primary rays —
their bits taken from the library itself: renderFeatures' `dir` per pixel under the selected policy, the origin camera[0:3]
— must give rt_render_spp's accumulator bit for bit, in every row of the queue family and in the fixed-lane family; a ray's
result must not depend on its slot, its neighbours or the batch's length; arbitrary rays are rt_trace_samples' (and, under
policy 0, the oracle's) radiances; the accumulator target, the moments, the feature records and the state rules are those
of rt_render_spp_cameras."""
import ctypes as C

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


def primary_batch(t, camera):
    """The camera's primary rays with the selected policy's own direction bits, ids = pixel coordinates → RAY (h * w,)."""
    t.renderFeatures(camera)
    rec = t.featureRecords()
    h, w = rec.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return rays_mod.pack_rays(np.asarray(camera, np.float32)[0:3], rec["dir"].reshape(-1, 3),
                              ids=np.stack([xs.ravel(), ys.ravel()], axis=1))


def to_device(batch):
    import torch
    return torch.from_numpy(rays_mod.as_floats(batch).copy()).cuda()


def render_batch(t, batch, first, n):
    """renderRays of a host batch as a torch tensor into a zeroed external buffer → (len(batch), 4) float32"""
    import torch
    d = to_device(batch)
    out = torch.zeros((len(batch), 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t.renderRays(d, first, n, out=out)
    t.sync()
    return out.cpu().numpy()


def frame_accum(t, camera, first, n):
    t.clear()
    t.renderSamples(camera, first, n)
    return read_accum(t).reshape(-1, 4)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- 1. frame parity, all five queue rows, every policy ---------------------------------------------------------------------
SCENES = {   # workload, its arguments at 48 x 27 → the (ACCEL, GEOM) row of the queue its launches must run
    "c2": (dict(), (0, 0)),
    "all_kinds": (dict(), (0, 1)),
    "c3": (dict(tex_size=64), (0, 1)),                     # a few small meshes: their faces in LDS
    "c4": (dict(n_spheres=3000), (1, 0)),                  # a crop of C4: the sphere BVH
    "c5": (dict(segments=24, rings=16), (1, 2)),           # a crop of C5: the mesh BVH
}


def workload(name):
    kw, row = SCENES[name]
    return rt.workloads.get(name, width=W, height=H, **kw), row


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_frame_parity_in_every_queue_row(name, policy):
    wl, row = workload(name)
    t = tracer(wl, policy)
    try:
        batch = primary_batch(t, wl.camera)
        for n in (1, 3, 64, 512):
            want = frame_accum(t, wl.camera, 0, n)
            got = render_batch(t, batch, 0, n)
            facts, plan = t.lastRayPlan()
            assert (plan["family"], plan["accel"], plan["geom"]) == (QUEUE,) + row, (name, n, plan)
            assert plan == R.plan_camera_samples(**facts) and facts["n"] == W * H and facts["count"] == n
            if name == "c3":
                assert plan["lds_face_f4"] > 0
            assert (want[:, 3] == n).all() and want[:, :3].any()
            assert same_bits(got, want), (name, policy, n)
        assert t.walkOverflow() == 0
    finally:
        t.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_520_samples_are_two_launches_and_a_first_sample_of_7(policy):
    wl, _ = workload("c2")
    t = tracer(wl, policy)
    try:
        batch = primary_batch(t, wl.camera)
        want = frame_accum(t, wl.camera, 0, 520)
        got = render_batch(t, batch, 0, 520)
        facts, _ = t.lastRayPlan()
        assert facts["count"] == 8 and (want[:, 3] == 520).all()
        assert same_bits(got, want)
        want = frame_accum(t, wl.camera, 7, 24)
        assert same_bits(render_batch(t, batch, 7, 24), want)
        assert not same_bits(frame_accum(t, wl.camera, 0, 24), want)   # (the first sample says something)
    finally:
        t.close()


@pytest.mark.parametrize("queue", [1, 0])
def test_three_slot_ranges_change_no_bit(queue):
    """A plain ray call cut into slot ranges (RT_OPT_MAX_THREADS_PER_LAUNCH): 24 samples are 32 lanes per ray, so W * H * 32 // 3
    + 64 threads are 434 rays per range — three ranges, the last one of 428 rays — in the queue and in the fixed-lane family."""
    wl, _ = workload("c2")
    n = 24
    threads = W * H * 32 // 3 + 64
    t = tracer(wl, 2, OPT_SAMPLE_QUEUE=queue)
    try:
        batch = primary_batch(t, wl.camera)
        want = render_batch(t, batch, 0, n)
        facts, plan = t.lastRayPlan()
        assert facts["n"] == W * H and plan["family"] == (QUEUE if queue else FIXED) and want[:, :3].any()
        t.setOption(T.OPT_MAX_THREADS_PER_LAUNCH, threads)
        got = render_batch(t, batch, 0, n)
        facts, plan = t.lastRayPlan()
        assert facts["n"] < W * H and facts["n"] == W * H - 2 * (threads >> 5), "the last of three slot ranges"
        assert plan["family"] == (QUEUE if queue else FIXED)
        assert same_bits(got, want)
    finally:
        t.close()


# ---- 2. mixed batch and slot independence --------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_mixed_batch_and_slot_independence(policy):
    wl, _ = workload("c2")
    aspect = np.float32(W) / np.float32(H)
    glass = wl.scene.spheres[[m["type"] in (A.T_DIELECTRIC, A.T_REFRACTIVE) for m in wl.scene.materials[wl.scene.spheres["mat_ID"]]]]
    assert len(glass), "C2 has a glass sphere"
    cams = [wl.camera, rt.Camera(60, aspect, (-6, -2, -9), 30.0, 5.0).transferData(),
            rt.Camera(60, aspect, tuple(glass[0]["pos"][:3]), 45.0, 0.0).transferData()]   # the last one looks out of the glass
    n = 16
    t = tracer(wl, policy)
    try:
        batches = [primary_batch(t, c) for c in cams]
        frames = [frame_accum(t, c, 0, n) for c in cams]
        assert not same_bits(frames[0], frames[2]) and not same_bits(frames[0], frames[1])
        cut = 3 * W * H - 5                                  # not a multiple of any wave's pixels
        full = np.concatenate(batches)[:cut]
        want = np.concatenate(frames)[:cut]
        got = render_batch(t, full, 0, n)
        assert same_bits(got, want)
        perm = np.random.RandomState(5).permutation(cut)
        got_p = render_batch(t, full[perm], 0, n)
        assert same_bits(got_p, got[perm])
        for k in (1, 65):
            pick = perm[:k]
            assert same_bits(render_batch(t, full[pick], 0, n), want[pick]), k
    finally:
        t.close()


# ---- 3. arbitrary rays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_arbitrary_rays_are_trace_samples(policy, oracle, table):
    wl, _ = workload("c2")
    rng = np.random.RandomState(11)
    n = 32
    o = (rng.uniform(-9.0, 9.0, (n, 3)) + 0.0137).astype(np.float32)
    d = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    d[np.abs(d) < 0.05] = 0.25
    assert (o != 0).all() and (d != 0).all()
    ids = np.stack([rng.randint(0, W, n), rng.randint(0, H, n)], axis=1)
    t = tracer(wl, policy)
    try:
        # the degenerate camera {o, d, 0, 0, 0, 0, 0, 0}: its primary ray at every pixel is (o, normalize(d))
        cams = np.zeros((n, 12), np.float32)
        cams[:, 0:3], cams[:, 3:6] = o, d
        dirs = np.empty((n, 3), np.float32)
        for i in range(n):
            t.renderFeatures(cams[i])
            rec = t.featureRecords()
            dirs[i] = rec["dir"][ids[i, 1], ids[i, 0]]
            assert same_bits(rec["dir"], np.broadcast_to(dirs[i], rec["dir"].shape))
        batch = rays_mod.pack_rays(o, dirs, ids=ids)
        hit_something = False
        for s in (0, 5):
            got = render_batch(t, batch, s, 1)
            assert (got[:, 3] == 1).all()
            want = np.stack([t.traceSamples(cams[i], [ids[i, 0]], [ids[i, 1]], [s])[0] for i in range(n)])
            want = (np.float32(0) + want).astype(np.float32)            # (a one-sample group's sum: 0.0f + radiance)
            assert same_bits(got[:, :3], want), s
            hit_something |= bool(want.any())
            if policy == 0:
                exp = np.stack([oracle.samples(wl.scene, cams[i], table, W, H, ids[i:i + 1, 0], ids[i:i + 1, 1], np.array([s]))[0][0]
                                for i in range(n)])
                assert same_bits(got[:, :3], (np.float32(0) + exp).astype(np.float32)), s
        assert hit_something
    finally:
        t.close()


# ---- 4. the fixed-lane family -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["c2", "c5"])
def test_fixed_lane_family(name, policy):
    wl, _ = workload(name)
    n = 24
    t = tracer(wl, policy)
    try:
        batch = primary_batch(t, wl.camera)
        want = frame_accum(t, wl.camera, 0, n)
        t.setOption(T.OPT_SAMPLE_QUEUE, 0)
        got = render_batch(t, batch, 0, n)
        assert t.lastRayPlan()[1]["family"] == FIXED and same_bits(got, want)
        t.setOption(T.OPT_SAMPLE_QUEUE, 1)
        t.enableCounters(True)
        t.resetCounters()
        got = render_batch(t, batch, 0, n)
        mine = t.counters().as_dict()
        _, plan = t.lastRayPlan()
        assert plan["family"] == FIXED and plan["count"] == 1 and same_bits(got, want)
        t.resetCounters()
        t.clear()
        t.renderSamplesCameras(np.tile(wl.camera, (n, 1)), 0)
        t.sync()
        theirs = t.counters().as_dict()
        assert mine == theirs and mine["samples"] == W * H * n and mine["bounces"] > 0
    finally:
        t.close()


# ---- 5. the accumulator as the target -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_accumulator_target_and_resolve(policy):
    wl, _ = workload("c2")
    t = tracer(wl, policy)
    try:
        batch = primary_batch(t, wl.camera)
        t.clear()
        t.renderSamples(wl.camera, 0, 32)
        one = read_accum(t)
        t.renderSamples(wl.camera, 32, 32)
        t.resolve()
        two, image = read_accum(t), t.transferImage()
        t.uploadRays(batch)
        t.clear()
        t.renderRays(None, 0, 32)
        assert same_bits(read_accum(t), one)
        t.renderRays(None, 32, 32)
        t.resolve()
        assert same_bits(read_accum(t), two) and same_bits(t.transferImage(), image)
        assert (t.sampleCounts() == 64).all()
    finally:
        t.close()


def test_moments_follow_the_camera_call():
    w, h, n = 24, 16, 24
    wl = rt.workloads.get("c2", width=w, height=h)
    t = tracer(wl)
    try:
        batch = primary_batch(t, wl.camera)
        ys, xs = np.mgrid[0:h, 0:w]
        s = t.traceSamples(wl.camera, np.repeat(xs.reshape(-1), n), np.repeat(ys.reshape(-1), n), np.tile(np.arange(n), w * h))
        lum = (s.astype(np.float64) @ V.LUM).reshape(h, w, n)
        truth = ((lum - lum.mean(-1, keepdims=True)) ** 2).sum(-1)
        tol = M.tolerance(truth, np.full((h, w), n), lum.max(-1))
        t.uploadRays(batch)
        got = []
        for on in (0, 1):
            t.setOption(T.OPT_MOMENTS, on)
            t.clear()
            t.renderRays(None, 0, n)
            t.resolve()
            got.append((read_accum(t), t.transferImage()))
            if on:
                assert t.lastRayPlan()[1]["family"] == FIXED and t.lastRayPlan()[1]["moments"] == 1
        assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])     # the option moves no bit
        mine = t.moments()
        t.clear()
        t.renderSamplesCameras(np.tile(wl.camera, (n, 1)), 0)
        assert same_bits(read_accum(t), got[1][0])
        theirs = t.moments()
        for m2, what in ((mine, "rays"), (theirs, "cameras")):
            err = np.abs(m2.astype(np.float64) - truth)
            print("%s: max |M2 - truth| %.3g (largest tolerance %.3g, max M2 %.4g)" % (what, err.max(), tol.max(), truth.max()))
            assert (err <= tol).all() and (m2 >= 0).all(), what
        assert (np.abs(mine.astype(np.float64) - theirs) <= tol).all() and truth.max() > 0
    finally:
        t.close()


# ---- 6. feature records -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_feature_records(policy):
    wl, _ = workload("c2")
    t = tracer(wl, policy)
    try:
        batch = primary_batch(t, wl.camera)
        d = to_device(batch)
        import torch
        torch.cuda.synchronize()
        for follow, chain in ((0, 0), (R.FOLLOW_ALL, 29)):
            t.renderFeaturesChain(wl.camera, follow, chain)
            want = t.featureRecords()
            t.renderFeatures(np.zeros(12, np.float32) + np.float32(1))      # (something else in the records)
            t.renderFeaturesRays(d, follow, chain)
            got = t.featureRecords()
            assert got.tobytes() == want.tobytes(), (follow, chain)
            assert (want["flags"] & A.FEATURE_HIT).any()
        assert ((want["flags"] >> 8) & 31).max() > 0                         # C2's mirror and glass were followed
        t.clear()
        t.renderRays(d, 0, 8)
        img = t.denoise()
        assert np.isfinite(img).all() and img[..., :3].any()
    finally:
        t.close()


# ---- 7. state and errors ----------------------------------------------------------------------------------------------------
def test_errors_change_nothing():
    import torch
    wl, _ = workload("c2")
    t = tracer(wl)
    lib = R.load_library()
    try:
        batch = primary_batch(t, wl.camera)
        n = len(batch)
        d = to_device(batch)
        out = torch.full((n, 4), 3.0, dtype=torch.float32, device="cuda")
        t.clear()
        t.renderSamples(wl.camera, 0, 4)
        before = read_accum(t)
        torch.cuda.synchronize()
        dp, op = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
        call = lib.rt_render_rays
        assert call(None, dp, n, 0, 4, op) == EINVAL
        assert call(t._ctx, dp, 0, 0, 4, op) == EINVAL                        # no rays
        assert call(t._ctx, dp, (1 << 28) + 1, 0, 4, op) == EINVAL            # too many
        assert call(t._ctx, dp, n, 65533, 4, op) == EINVAL                    # sample 65536
        assert call(t._ctx, None, n, 0, 4, op) == EINVAL                      # nothing uploaded
        assert call(t._ctx, dp, n - 1, 0, 4, None) == EINVAL                  # the accumulator wants W * H rays
        t.uploadRays(batch[:n - 1])
        assert t.deviceRays()[1] == n - 1
        assert call(t._ctx, None, n, 0, 4, op) == EINVAL                      # fewer uploaded than asked for
        assert lib.rt_render_features_rays(t._ctx, dp, n - 1, None) == EINVAL
        assert lib.rt_render_features_rays(t._ctx, None, n, None) == EINVAL
        assert lib.rt_upload_rays(t._ctx, None, 4) == EINVAL and lib.rt_upload_rays(t._ctx, batch.ctypes.data, 0) == EINVAL
        t.setShard(0, 2, 8, 8)
        assert call(t._ctx, dp, n, 0, 4, op) == EINVAL                        # a sharded context
        assert lib.rt_render_features_rays(t._ctx, dp, n, None) == EINVAL
        t.setShard(0, 1, 8, 8)
        with pytest.raises(ValueError):
            t.renderRays(d[:, :6], 0, 1)
        with pytest.raises(ValueError):
            t.renderRays(d.cpu(), 0, 1)
        with pytest.raises(ValueError):
            t.renderRays(d, 0, 1, out=out[:-1])
        f, p = A.CameraFacts(), A.CameraPlan()
        assert lib.rt_debug_last_ray_plan(t._ctx, C.byref(f), C.byref(p)) == EINVAL   # no ray launch yet: every call failed
        assert same_bits(read_accum(t), before) and (out.cpu().numpy() == 3.0).all()
        assert call(t._ctx, dp, n, 65532, 4, op) == 0                         # sample 65535 is the last
        assert call(t._ctx, dp, n, 0, 0, op) == 0                             # nothing to do
        t.sync()
        ctx = C.c_void_p()
        assert lib.rt_create(0, W, H, C.byref(ctx)) == 0
        assert call(ctx, dp, n, 0, 4, op) == ESTATE                           # no scene
        assert lib.rt_render_features_rays(ctx, dp, n, None) == ESTATE
        lib.rt_destroy(ctx)
    finally:
        t.close()


def test_a_ray_call_leaves_the_other_state_alone():
    wl, _ = workload("c2")

    def sequence(with_rays):
        t = tracer(wl)
        batch = primary_batch(t, wl.camera)
        t.renderFeatures(wl.camera)
        images = []
        t.clear()
        t.renderSamples(wl.camera, 0, 16)           # leaves a kept prefix
        t.render(wl.camera)
        t.renderAgain(wl.camera)
        t.renderAgain(wl.camera)                    # the second call at rest: a look-ahead batch is pending
        images.append(t.transferImage())
        if with_rays:
            assert render_batch(t, batch, 0, 8)[:, 3].min() == 8
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


# ---- 8. panorama smoke ------------------------------------------------------------------------------------------------------
def test_equirect_panorama():
    w, h = 64, 32
    wl = rt.workloads.get("c2", width=w, height=h)
    pano = rays_mod.equirect_rays(wl.camera[0:3], w, h, yaw=45.0)
    t = tracer(wl)
    try:
        assert t.uploadRays(pano) == w * h
        t.clear()
        t.renderRays(None, 0, 32)
        t.resolve()
        img, acc = t.transferImage(), read_accum(t)
        assert np.isfinite(img).all() and (acc[..., 3] == 32).all()
        lit = img[..., :3].sum(-1).reshape(h, w)
        assert (lit > 0).any(axis=1).sum() >= h // 2, "rows that face the lights are not black"
        t.clear()
        import torch
        d = to_device(pano)
        torch.cuda.synchronize()
        t.renderRays(d, 0, 32)
        assert same_bits(read_accum(t), acc)
    finally:
        t.close()


# ---- 9. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_projection_matches_the_python_path(built, tmp_path):
    import os
    import subprocess
    w, h, spp = 64, 40, 8
    scene = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    raw, raw_dn = str(tmp_path / "f.f32"), str(tmp_path / "d.f32")
    base = [os.path.join(cases.ROOT, "host", "rt_cli"), "--scene", scene, "--size", "%dx%d" % (w, h), "--spp", str(spp),
            "--camera=-8,-1,-8,45,0", "--projection", "ortho", "--extent", "12"]
    subprocess.run(base + ["--raw", raw], check=True, cwd=cases.ROOT)
    out = subprocess.run(base + ["--raw", raw_dn, "--denoise"], check=True, cwd=cases.ROOT, capture_output=True, text=True).stdout
    assert "caller-supplied rays" in out and "denoised" in out
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    got_dn = np.fromfile(raw_dn, np.float32).reshape(h, w, 4)
    s = rt.SceneCreator()
    s.loadScene(scene, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        t.uploadRays(rays_mod.orthographic_rays((-8, -1, -8), w, h, 12.0, 45.0, 0.0))
        t.clear()
        t.renderRays(None, 0, spp)
        t.resolve()
        exp = t.transferImage()
        t.renderFeaturesRays(None)
        exp_dn = t.denoise()
    finally:
        t.close()
    # Both hosts do the trigonometry in double and round once: a ray differs between them only where a double lies within
    # an ulp of a float32 rounding boundary (about 1e-8 per component), and a pixel only through its ray
    assert np.isfinite(got).all() and got[..., :3].any()
    assert (got.view(np.uint32) == exp.view(np.uint32)).all(-1).mean() >= 0.99
    assert np.isfinite(got_dn).all() and np.abs(got_dn - exp_dn).mean() <= 1e-3
    # the usage rules: a projection is one way to spend the samples
    assert subprocess.run(base + ["--aa"], cwd=cases.ROOT, capture_output=True).returncode == 2
    assert subprocess.run(base + ["--fov-deg", "90"], cwd=cases.ROOT, capture_output=True).returncode == 2
