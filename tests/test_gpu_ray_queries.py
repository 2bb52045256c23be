"""GPU (-m gpu): the ray queries rt_intersect_rays and rt_occluded_rays.  Nearest hits for any batch are the records
rt_render_features_rays writes, bit for bit and whatever the slot, and move nothing of the context; a record is occluded
iff its first hit's t is below its bound in binary32 — checked against the library's own first hits under every policy,
against the CPU oracle under policy 0, at the bounds where an early exit could go wrong (t itself and its two neighbours,
NaN, 0, negative, MIN_DISTANCE, MAX_DISTANCE), on origins that lie on surfaces, on directions that are not unit, on a mesh
whose first face in face order is not its nearest, and as counts over sets that straddle waves and workgroups."""
import ctypes as C

import numpy as np
import pytest

import cases
import ray_queries_ref as Q

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
R = rt.raytracer
T = rt.RayTracer
rays_mod = rt.rays
F32 = np.float32
EINVAL, ESTATE = -1, -4
W, H = 48, 27
POLICIES = [0, 1, 2]
SCENES = {   # the five rows of tests/test_gpu_rays.py
    "c2": dict(),
    "all_kinds": dict(),
    "c3": dict(tex_size=64),
    "c4": dict(n_spheres=3000),               # a sphere BVH
    "c5": dict(segments=24, rings=16),        # a mesh BVH
}
POISON = 0xDEADBEEF


def workload(name):
    return rt.workloads.get(name, width=W, height=H, **SCENES[name])


def tracer(wl, policy=0, **options):
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    if policy:
        t.setArith(policy)
    for k, v in options.items():
        t.setOption(getattr(T, k), v)
    return t


def to_device(batch):
    import torch
    return torch.from_numpy(rays_mod.as_floats(batch).copy()).cuda()


def primary_batch(t, camera):
    """The camera's primary rays with the selected policy's own direction bits → RAY (h * w,)"""
    t.renderFeatures(camera)
    rec = t.featureRecords()
    ys, xs = np.mgrid[0:rec.shape[0], 0:rec.shape[1]]
    return rays_mod.pack_rays(np.asarray(camera, F32)[0:3], rec["dir"].reshape(-1, 3), ids=np.stack([xs.ravel(), ys.ravel()], axis=1))


def intersect(t, batch, follow=0, max_chain=0):
    """intersectRays of a host batch as a device tensor → (n,) FEATURE"""
    import torch
    d = to_device(batch)
    torch.cuda.synchronize()
    out = t.intersectRays(d, follow, max_chain)
    t.sync()
    return A.feature_records(out)


def occluded(t, batch, set_size=1, t_max=float("inf"), bounds=None):
    """occludedRays of a host batch as a device tensor into a poisoned output → (n_sets,) uint32"""
    import torch
    d = to_device(batch)
    n = len(np.asarray(batch).reshape(-1)) // set_size
    out = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device="cuda")
    b = None if bounds is None else torch.from_numpy(np.ascontiguousarray(bounds, dtype=F32)).cuda()
    torch.cuda.synchronize()
    got = t.occludedRays(d, set_size, t_max, b, out=out)
    t.sync()
    assert got is out
    return out.cpu().numpy().view(np.uint32)


def query_batch(t, camera, seed=11):
    """The rays an occlusion query meets: the primary batch, one cosine-hemisphere ray from every hit point (its origin ON
    the surface), and copies of both with the directions scaled by 1.1 and by 2 (the latter leave the sphere BVH for the
    brute-force loop) → RAY (n,)"""
    prim = primary_batch(t, camera)
    rec = intersect(t, prim)
    hit = (rec["flags"] & A.FEATURE_HIT) != 0
    assert hit.any()
    hemi = rays_mod.hemisphere_sets(rec["pos"][hit], rec["normal"][hit], 1, seed).reshape(-1)
    base = np.concatenate([prim, hemi])
    out = [base]
    for scale in (F32(1.1), F32(2.0)):
        c = base.copy()
        c["d"] = (base["d"] * scale).astype(F32)
        out.append(c)
    return np.concatenate(out)


# ---- 1. nearest hits: rt_render_features_rays' records, any batch, nothing else moves ----------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_intersect_is_the_feature_record_of_every_ray(name, policy):
    import torch
    wl = workload(name)
    t = tracer(wl, policy)
    lib = R.load_library()
    try:
        fresh = tracer(wl, policy)
        try:                                               # a fresh context has no feature records, before and after
            few = rays_mod.pack_rays(np.asarray(wl.camera, F32)[0:3], np.array([[0, 0, 1], [0, 1, 0]], F32))
            assert len(intersect(fresh, few)) == 2
            buf = np.empty((H, W), dtype=A.FEATURE)
            assert lib.rt_read_features(fresh._ctx, buf.ctypes.data, buf.nbytes) == ESTATE
        finally:
            fresh.close()
        batch = primary_batch(t, wl.camera)
        d = to_device(batch)
        torch.cuda.synchronize()
        for follow, chain in ((0, 0), (R.FOLLOW_ALL, 4)):
            t.renderFeaturesRays(d, follow, chain)
            want = t.featureRecords()
            got = intersect(t, batch, follow, chain)
            assert got.tobytes() == want.tobytes(), (name, policy, follow)
            assert t.featureRecords().tobytes() == want.tobytes()          # the context's records did not move
            assert (want["flags"] & A.FEATURE_HIT).any()
            flat = want.reshape(-1)
            for n in (1, 63, 65, 257):                                     # sub-batches from the middle of the frame
                first = (W * H - n) // 2 + 3
                sub = intersect(t, batch[first:first + n], follow, chain)
                assert sub.tobytes() == flat[first:first + n].tobytes(), (name, policy, follow, n)
        t.uploadRays(batch[5:70])                                          # NULL d_rays: the uploaded rays
        out = t.intersectRays(None)
        t.sync()
        t.renderFeaturesRays(d)
        assert A.feature_records(out).tobytes() == t.featureRecords().reshape(-1)[5:70].tobytes()
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 2. occlusion is its definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_occluded_is_first_hit_below_the_bound(name, policy):
    wl = workload(name)
    t = tracer(wl, policy)
    try:
        batch = query_batch(t, wl.camera)
        rec = intersect(t, batch)
        tt = rec["t"].astype(F32)
        hit = (rec["flags"] & A.FEATURE_HIT) != 0
        assert np.isinf(tt[~hit]).all() and np.isfinite(tt[hit]).all() and hit.any()
        third = len(batch) // 3
        assert hit[third:].any() and hit[2 * third:].any()                 # the scaled copies hit things too
        bounds = Q.cycled_bounds(tt)
        want = Q.occluded(tt, bounds)
        got = occluded(t, batch, bounds=bounds)
        print(name, policy, "records", len(batch), "hits", int(hit.sum()), "occluded", int(want.sum()), "differ", int((got != want).sum()))
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), want), np.flatnonzero(got.astype(bool) != want)[:10]
        assert want.any() and (~want[hit]).any()
        any_hit = occluded(t, batch)                                       # bounds None, t_max +inf: the hit flag
        assert np.array_equal(any_hit.astype(bool), hit)
        near = occluded(t, batch, t_max=3.0)                               # one bound for every record
        assert np.array_equal(near.astype(bool), Q.occluded(tt, F32(3.0)))
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 3. a mesh reports its first front-facing face in face order, not its nearest -------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("accel", [0, 1])
def test_face_order_rule(accel, policy):
    scene = Q.face_order_scene()
    t = T(W, H, scene=scene, seed=cases.SEED)
    try:
        if policy:
            t.setArith(policy)
        t.setOption(T.OPT_ACCEL, accel)
        ray = rays_mod.pack_rays(Q.FACE_ORDER_RAY[:3], Q.FACE_ORDER_RAY[None, 3:])
        rec = intersect(t, ray)
        assert rec["t"][0] == F32(6.0) and rec["face"][0] == 0
        side = rays_mod.pack_rays((50, 0, 0), Q.FACE_ORDER_RAY[None, 3:])
        assert intersect(t, side)["t"][0] == F32(5.0)
        for bound, want in Q.FACE_ORDER_CASES:
            assert bool(occluded(t, ray, t_max=bound)[0]) is want, (accel, policy, bound)
            assert bool(occluded(t, ray, bounds=np.array([bound], F32))[0]) is want
        # among 70 rays (two waves), so that lanes with and without an answer share a walk
        many = np.concatenate([ray, side] * 35)
        got = occluded(t, many, bounds=np.tile(np.array([4.0, 5.5], F32), 35))
        assert np.array_equal(got, np.tile(np.array([0, 1], np.uint32), 35))
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 4. sets: counts over runs of lanes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [0, 2])
@pytest.mark.parametrize("name", ["all_kinds", "c4"])
def test_set_counts_are_sums_of_the_single_records(name, policy):
    wl = workload(name)
    t = tracer(wl, policy)
    n_sets = 37
    try:
        batch = query_batch(t, wl.camera)
        pick = (np.arange(n_sets * 100) * 2) % len(batch)                  # primary and hemisphere rays, hits and misses
        batch = batch[pick]
        bounds = Q.cycled_bounds(intersect(t, batch)["t"])
        single = occluded(t, batch, bounds=bounds)
        single_inf = occluded(t, batch)
        assert 0 < single.sum() < len(batch) and set(np.unique(single)) <= {0, 1}
        for k in (1, 3, 64, 100):
            m = n_sets * k
            got = occluded(t, batch[:m], set_size=k, bounds=bounds[:m])
            assert np.array_equal(got, single[:m].reshape(n_sets, k).sum(1)), (name, policy, k)
            got = occluded(t, batch[:m].reshape(n_sets, k), set_size=k)
            assert np.array_equal(got, single_inf[:m].reshape(n_sets, k).sum(1)), (name, policy, k)
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 5. options and state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["c4", "c5"])
def test_accel_changes_no_bit(name, policy):
    wl = workload(name)
    results = []
    for accel in (0, 1, 2):
        t = tracer(wl, policy, OPT_ACCEL=accel)
        try:
            if not results:
                batch = query_batch(t, wl.camera)
                bounds = Q.cycled_bounds(intersect(t, batch)["t"])
            results.append((intersect(t, batch).tobytes(), occluded(t, batch, bounds=bounds).tobytes(),
                            occluded(t, batch[:3 * 700], set_size=3).tobytes()))
            assert t.walkOverflow() == 0
        finally:
            t.close()
    assert results[0] == results[1] == results[2]


def test_the_queries_move_no_state():
    import torch
    wl = workload("all_kinds")
    t = tracer(wl, 2, OPT_MOMENTS=1)
    try:
        batch = query_batch(t, wl.camera)
        t.clear()
        t.renderSamples(wl.camera, 0, 4)
        t.resolve()

        def state():
            t.sync()
            accum = torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()
            return accum.tobytes(), t.transferImage().tobytes(), t.sample_counter, t.moments().tobytes(), t.featureRecords().tobytes()

        before = state()
        intersect(t, batch, R.FOLLOW_ALL, 4)
        occluded(t, batch)
        occluded(t, batch[:64 * 30], set_size=64, t_max=2.0)
        assert state() == before
        t.renderSamples(wl.camera, 4, 4)                                   # and the frame goes on as if nothing had happened
        t.resolve()
        after = state()
        t.clear()
        t.renderSamples(wl.camera, 0, 4)
        t.renderSamples(wl.camera, 4, 4)
        t.resolve()
        want = state()
        assert after[0] == want[0] and after[1] == want[1] and after[3] == want[3]
    finally:
        t.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    import torch
    wl = workload("c2")
    t = tracer(wl)
    lib = R.load_library()
    try:
        batch = primary_batch(t, wl.camera)
        n = len(batch)
        d = to_device(batch)
        rec = torch.full((n, A.FEATURE_FLOATS), 3.0, dtype=torch.float32, device="cuda")
        cnt = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        tm = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dp, rp, cp, tp = (C.c_void_p(x.data_ptr()) for x in (d, rec, cnt, tm))
        inf = C.c_float(float("inf"))
        P = A.FeatureChainParams

        def prefill_holds():
            t.sync()
            torch.cuda.synchronize()
            return bool((rec == 3.0).all()) and bool((cnt == 7).all())

        def hit(*args):                                                             # a refused call: its code, and nothing written
            rc = lib.rt_intersect_rays(*args)
            assert rc != 0 and prefill_holds(), ("rt_intersect_rays wrote", args[2:4])
            return rc

        def occ(*args):
            rc = lib.rt_occluded_rays(*args)
            assert rc != 0 and prefill_holds(), ("rt_occluded_rays wrote", args[2:4])
            return rc

        assert hit(None, dp, n, None, rp) == EINVAL
        assert hit(t._ctx, dp, n, None, None) == EINVAL                              # no output
        assert hit(t._ctx, dp, n, None, C.c_void_p(rec.data_ptr() + 4)) == EINVAL    # misaligned output
        assert hit(t._ctx, C.c_void_p(d.data_ptr() + 4), n - 1, None, rp) == EINVAL  # misaligned rays
        assert hit(t._ctx, dp, 0, None, rp) == EINVAL
        assert hit(t._ctx, dp, (1 << 28) + 1, None, rp) == EINVAL
        assert hit(t._ctx, None, n, None, rp) == EINVAL                              # nothing uploaded
        assert hit(t._ctx, dp, n, C.byref(P(8, 1)), rp) == EINVAL                    # unknown follow bits
        assert hit(t._ctx, dp, n, C.byref(P(1, A.FEATURE_CHAIN_MAX + 1)), rp) == EINVAL
        assert occ(None, dp, n, 1, None, inf, cp) == EINVAL
        assert occ(t._ctx, dp, n, 1, None, inf, None) == EINVAL                      # no output
        assert occ(t._ctx, dp, 0, 1, None, inf, cp) == EINVAL
        assert occ(t._ctx, dp, (1 << 28) + 1, 1, None, inf, cp) == EINVAL
        assert occ(t._ctx, dp, n, 0, None, inf, cp) == EINVAL                        # set_size 0
        assert occ(t._ctx, dp, 1, A.RAY_SET_MAX + 1, None, inf, cp) == EINVAL
        assert occ(t._ctx, dp, (1 << 20) + 1, 2048, None, inf, cp) == EINVAL         # more than 2^31 records
        assert occ(t._ctx, C.c_void_p(d.data_ptr() + 8), n - 1, 1, None, inf, cp) == EINVAL
        assert occ(t._ctx, dp, n, 1, C.c_void_p(tm.data_ptr() + 2), inf, cp) == EINVAL   # misaligned bounds
        assert occ(t._ctx, dp, n, 1, None, inf, C.c_void_p(cnt.data_ptr() + 2)) == EINVAL
        assert occ(t._ctx, None, n, 1, None, inf, cp) == EINVAL                      # nothing uploaded
        t.uploadRays(batch[:n - 1])
        assert hit(t._ctx, None, n, None, rp) == EINVAL                              # fewer uploaded than asked for
        assert occ(t._ctx, None, n, 1, None, inf, cp) == EINVAL
        assert occ(t._ctx, None, n // 2, 2, None, inf, cp) == EINVAL                 # (n is even: n records, n - 1 uploaded)
        t.setShard(0, 2, 8, 8)
        assert hit(t._ctx, dp, n, None, rp) == EINVAL                                # a sharded context
        assert occ(t._ctx, dp, n, 1, None, inf, cp) == EINVAL
        t.setShard(0, 1, 8, 8)
        ctx = C.c_void_p()
        assert lib.rt_create(0, W, H, C.byref(ctx)) == 0
        assert hit(ctx, dp, n, None, rp) == ESTATE                                   # no scene
        assert occ(ctx, dp, n, 1, None, inf, cp) == ESTATE
        lib.rt_destroy(ctx)
        with pytest.raises(ValueError):
            t.intersectRays(d, out=rec[:-1])
        with pytest.raises(ValueError):
            t.occludedRays(d, out=cnt.float())
        with pytest.raises(ValueError):
            t.occludedRays(d, bounds=tm[:-1])
        with pytest.raises(ValueError):
            t.occludedRays(d, set_size=5)
        with pytest.raises(ValueError):                                              # bounds live on the device: a host array
            t.occludedRays(d, bounds=np.full(n, 5.0, F32), out=cnt)                  # is refused, not copied behind the caller's back
        assert prefill_holds()
        assert lib.rt_intersect_rays(t._ctx, dp, n, None, rp) == 0                   # and the same buffers are fine
        assert lib.rt_occluded_rays(t._ctx, dp, n, 1, tp, inf, cp) == 0
        t.sync()
        assert not (rec.cpu().numpy() == 3.0).all() and set(np.unique(cnt.cpu().numpy())) <= {0, 1}
    finally:
        t.close()


def test_device_memory_helpers():
    """rt_device_alloc / rt_device_copy / rt_device_free, what the C++ façade gets its buffers from: a round trip, a query
    into such a block, and the refusals."""
    wl = workload("c2")
    t = tracer(wl)
    lib = R.load_library()
    try:
        batch = primary_batch(t, wl.camera)
        want = occluded(t, batch)
        n = len(batch)
        host = np.arange(1000, dtype=np.uint32)
        back = np.zeros_like(host)
        p = C.c_void_p()
        assert lib.rt_device_alloc(t._ctx, host.nbytes, C.byref(p)) == 0 and p.value
        assert lib.rt_device_copy(t._ctx, p, host.ctypes.data, host.nbytes, 1) == 0
        assert lib.rt_device_copy(t._ctx, back.ctypes.data, p, host.nbytes, 0) == 0
        assert np.array_equal(back, host)
        assert lib.rt_device_free(t._ctx, p) == 0 and lib.rt_device_free(t._ctx, None) == 0
        counts = C.c_void_p()
        assert lib.rt_device_alloc(t._ctx, 4 * n, C.byref(counts)) == 0
        t.uploadRays(batch)
        assert lib.rt_occluded_rays(t._ctx, None, n, 1, None, C.c_float(float("inf")), counts) == 0
        got = np.zeros(n, np.uint32)
        assert lib.rt_device_copy(t._ctx, got.ctypes.data, counts, 4 * n, 0) == 0   # (behind the query on the stream)
        assert np.array_equal(got, want)
        assert lib.rt_device_free(t._ctx, counts) == 0
        q = C.c_void_p()
        assert lib.rt_device_alloc(None, 16, C.byref(q)) == EINVAL and lib.rt_device_alloc(t._ctx, 0, C.byref(q)) == EINVAL
        assert lib.rt_device_alloc(t._ctx, 16, None) == EINVAL and lib.rt_device_free(None, None) == EINVAL
        assert lib.rt_device_copy(t._ctx, None, host.ctypes.data, 4, 1) == EINVAL
        assert lib.rt_device_copy(t._ctx, back.ctypes.data, None, 4, 0) == EINVAL
        assert lib.rt_device_copy(None, back.ctypes.data, host.ctypes.data, 4, 0) == EINVAL
    finally:
        t.close()


# ---- 7. policy 0 against the CPU oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_policy_0_is_the_oracles_hit_scene(name, oracle):
    wl = workload(name)
    t = tracer(wl, 0)
    try:
        rays6 = Q.box_rays(wl.scene, 300, 900 + sorted(SCENES).index(name))
        batch = rays_mod.pack_rays(rays6[:, :3], rays6[:, 3:])
        t_ref = Q.first_hit_t(oracle, wl.scene, rays6)
        assert np.isfinite(t_ref).sum() >= 30
        assert np.array_equal(intersect(t, batch)["t"].view(np.uint32), t_ref.view(np.uint32))
        bounds = Q.cycled_bounds(t_ref)
        assert np.array_equal(occluded(t, batch, bounds=bounds).astype(bool), Q.occluded(t_ref, bounds))
        assert np.array_equal(occluded(t, batch).astype(bool), np.isfinite(t_ref))
        assert np.array_equal(occluded(t, batch[:297], set_size=3), np.isfinite(t_ref[:297]).reshape(99, 3).sum(1))
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 8. the C++ façade and rt_cli --ao ----------------------------------------------------------------------------------------
def test_cli_ambient_occlusion_is_the_python_path(built, tmp_path):
    """rt_cli --aov P --ao 8: first hits, rays::hemisphere_sets, RayTracer::occludedRays with set_size 8 → P_ao.pfm, against
    the same steps in Python.  The two hosts' sin / cos may differ in the last place of a direction, so a count may differ
    by one on a rare pixel: 99 % of the pixels equal, none off by more than 1 / 8."""
    import os
    import subprocess
    w, h, k = 96, 54, 8
    scene_file = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    prefix = str(tmp_path / "aov")
    cmd = [os.path.join(cases.ROOT, "host", "rt_cli"), "--scene", scene_file, "--size", "%dx%d" % (w, h), "--spp", "1",
           "--camera=-8,-1,-8,45,0", "--aov", prefix, "--ao", str(k), "--ao-distance", "4"]
    p = subprocess.run(cmd, check=True, cwd=cases.ROOT, capture_output=True, text=True)
    assert "ambient occlusion: 8 rays" in p.stdout
    raw = open(prefix + "_ao.pfm", "rb").read()
    head = b"Pf\n%d %d\n-1.0\n" % (w, h)
    assert raw.startswith(head)
    got = np.frombuffer(raw, np.float32, w * h, len(head))
    s = rt.SceneCreator()
    s.loadScene(scene_file, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        cam = rt.Camera(60, F32(w) / F32(h), (-8, -1, -8), 45.0, 0.0)
        t.renderFeatures(cam)
        rec = t.featureRecords().reshape(-1)
        hit = (rec["flags"] & A.FEATURE_HIT) != 0
        normal = rec["normal"][hit]
        facing = (normal * rec["dir"][hit]).sum(1, dtype=F32) > 0                # (float32, summed in the CLI's order)
        normal = np.where(facing[:, None], -normal, normal)
        sets = rays_mod.hemisphere_sets(rec["pos"][hit], normal, k, 0xC0FFEE)
        count = occluded(t, sets, set_size=k, t_max=4.0)
        want = np.ones(w * h, F32)
        want[hit] = F32(1) - count.astype(F32) / F32(k)
        assert hit.any() and (~hit).any() and 0 < count.sum() < count.size * k
        assert (got[~hit] == 1).all()
        assert (got == want).mean() >= 0.99 and np.abs(got - want).max() <= 1.0 / k + 1e-6
    finally:
        t.close()
