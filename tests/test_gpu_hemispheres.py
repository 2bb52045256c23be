"""GPU (-m gpu): hemisphere queries, rt_occluded_hemispheres.  The fused form's counts are, bit for bit, rt_occluded_rays'
counts over the very rays the spawn form dumps — under every policy and RT_OPT_ACCEL, for sets that cross waves and
workgroups, with records that have no hemisphere in between; the dumped rays are the float64 generator's (tests/
hemisphere_ref.py) to a bound taken from a measurement; nothing of the context moves; a refused call writes nothing;
ambientOcclusion and rt_cli --ao-device are 1 - count / K of the same call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import hemisphere_ref as HR

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
SCENES = {
    "c2": dict(),
    "all_kinds": dict(),
    "c4": dict(n_spheres=3000),               # a sphere BVH
    "c5": dict(segments=24, rings=16),        # a mesh BVH
}
POISON = 0xDEADBEEF
INF = float("inf")
# The bound on |component| of (device ray - float64 generator's ray, rounded to float32), origins and directions alike:
# 4 x the largest deviation measured on an MI355X over test_rays_are_the_float64_generators' records, all three policies
# (DESIGN.md §5 "Hemisphere queries": 2.4e-7, two float32 steps of a component near 1) — and it has to stay below 1e-5: one
# step of a 24-bit uniform moves a direction by 3.7e-7, a wrong counter, frame or sign by order 1.
MEASURED_MAX = 2.4e-7
RAY_BOUND = 4 * MEASURED_MAX
assert RAY_BOUND <= 1e-5


def workload(name):
    return rt.workloads.get(name, width=W, height=H, **SCENES[name])


def tracer(wl, policy=0, **options):
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    if policy:
        t.setArith(policy)
    for k, v in options.items():
        t.setOption(getattr(T, k), v)
    return t


def to_device(records):
    """(n,) FEATURE → (n, 20) float32 device tensor"""
    import torch
    flat = np.ascontiguousarray(np.asarray(records).reshape(-1)).view(F32).reshape(-1, A.FEATURE_FLOATS)
    d = torch.from_numpy(flat.copy()).cuda()
    torch.cuda.synchronize()
    return d


def first_hits(t, camera):
    """The first-hit records of the camera's primary rays → (h * w,) FEATURE (and the context then has feature records)"""
    t.renderFeatures(camera)
    return t.featureRecords().reshape(-1).copy()


def poisoned(n, k, counts=True, rays=True):
    import torch
    c = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device="cuda") if counts else None
    r = torch.full((n * k, 8), POISON - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32) if rays else None
    torch.cuda.synchronize()
    return c, r


def hemispheres(t, feats, k, counts=True, rays=True, **kw):
    """One rt_occluded_hemispheres call into poisoned outputs → (counts (n,) uint32 | None, rays (n, k) RAY | None, the
    device tensor of the rays | None)"""
    n = W * H if feats is None else int(feats.shape[0])
    c, r = poisoned(n, k, counts, rays)
    if counts:
        got = t.occludedHemispheres(feats, k, out=c, rays_out=r, **kw)
        assert got is c
    else:
        kw.pop("t_max", None)
        got = t.spawnHemispheres(feats, k, out=r, **kw)
        assert got is r
    t.sync()
    return (c.cpu().numpy().view(np.uint32) if counts else None,
            r.cpu().numpy().view(A.RAY).reshape(n, k) if rays else None, r)


def occluded(t, d_rays, k, t_max):
    import torch
    n = d_rays.shape[0] // k
    out = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t.occludedRays(d_rays, k, t_max, out=out)
    t.sync()
    return out.cpu().numpy().view(np.uint32)


def check_contract(t, feats, mask, k, t_max, tag, **kw):
    """counts with dump == counts without dump == occludedRays(dumped rays, k, t_max) on every valid record, 0 on the
    others, whose dumped records are zero bytes → (counts, rays)"""
    fused, none, _ = hemispheres(t, feats, k, True, False, t_max=t_max, **kw)
    both, dumped, d_rays = hemispheres(t, feats, k, True, True, t_max=t_max, **kw)
    assert none is None
    _, spawned, _ = hemispheres(t, feats, k, False, True, **kw)
    assert spawned.tobytes() == dumped.tobytes(), tag                      # the spawn form writes the same rays
    assert np.array_equal(fused, both), tag                                # the counts do not depend on the dump
    want = occluded(t, d_rays, k, t_max)
    assert np.array_equal(fused[mask], want[mask]), (tag, np.flatnonzero(fused != want)[:10])
    assert not fused[~mask].any() and not dumped[~mask].view(np.uint8).any(), tag
    assert fused.max() <= k
    return fused, dumped


# ---- 1. the exact contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_counts_are_the_occlusion_query_of_the_dumped_rays(name, policy, accel):
    wl = workload(name)
    t = tracer(wl, policy, OPT_ACCEL=accel)
    try:
        rec = first_hits(t, wl.camera)
        mask = HR.valid_mask(rec)
        assert mask.any()
        feats = to_device(rec)
        total = 0
        for k in (1, 5, 64, 100):
            for t_max in (INF, 1.0):
                counts, _ = check_contract(t, feats, mask, k, t_max, (name, policy, accel, k, t_max), seed=k, offset=1e-3,
                                           face_forward=True)
                total += int(counts.sum())
                print(name, policy, accel, "k", k, "t_max", t_max, "valid", int(mask.sum()), "occluded", int(counts.sum()), "of", int(mask.sum()) * k)
        assert total > 0                                                   # something occludes something
        # the context's own records (d_features NULL) are the same records
        own, _, _ = hemispheres(t, None, 5, True, False, seed=5, offset=1e-3, t_max=INF, face_forward=True)
        ext, _, _ = hemispheres(t, feats, 5, True, False, seed=5, offset=1e-3, t_max=INF, face_forward=True)
        assert np.array_equal(own, ext)
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 2. shapes where the run logic can break -----------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [0, 2])
@pytest.mark.parametrize("name", ["all_kinds", "c4"])
def test_sets_across_waves_and_workgroups_with_invalid_records_between(name, policy):
    wl = workload(name)
    t = tracer(wl, policy)
    try:
        base = first_hits(t, wl.camera)
        base = base[(base["flags"] & A.FEATURE_HIT) != 0]                 # hits only: the test places the invalid records itself
        sizes = (1, 5, 7, 100, 300)
        n = len(base)
        while any((n * k) % 256 == 0 for k in sizes):                      # no launch fills its last workgroup
            n -= 1
        base = base[:n]
        assert n >= 400
        for k in sizes:
            rec = base.copy()
            waves = np.arange((n * k + 63) // 64)
            bad = np.zeros(n, bool)
            step = 3 * max(1, k // 8)                                       # (every step-th wave: most records stay valid)
            bad[(64 * waves[waves % step == 0]) // k] = True               # the first record of a wave
            bad[np.minimum((64 * waves[waves % step == 1] + 63) // k, n - 1)] = True   # the last record of a wave
            bad[5::11] = True
            bad[n - 2] = False
            rec["flags"][bad] = 0
            rec["normal"][bad & (np.arange(n) % 2 == 0)] = 0                # some without a normal as well
            mask = HR.valid_mask(rec)
            assert np.array_equal(mask, ~bad) and (n * k) % 256 != 0 and mask[~bad].all()
            feats = to_device(rec)
            counts, dumped = check_contract(t, feats, mask, k, INF, (name, policy, k), seed=3, offset=1e-3, face_forward=True)
            # against the plain per-ray query, summed on the host: independent of any run logic
            single = occluded(t, to_device_rays(dumped), 1, INF).reshape(n, k)
            assert np.array_equal(counts[mask], single.sum(1)[mask]), (name, policy, k)
            assert 0 < counts.sum() < mask.sum() * k
            one, ray1 = check_contract(t, feats[n - 2:n - 1], np.array([True]), k, INF, (name, policy, k, "n=1"), seed=3, offset=1e-3,
                                       face_forward=True)
            assert one.shape == (1,) and ray1.shape == (1, k) and (ray1["x"] == 0).all()
        assert t.walkOverflow() == 0
    finally:
        t.close()


def to_device_rays(sets):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(sets).reshape(-1).view(F32).reshape(-1, 8).copy()).cuda()
    torch.cuda.synchronize()
    return d


# ---- 3. the generator ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator_reference():
    """records, and per (seed, offset, face_forward) the float64 generator's rays: computed once, shared by the policies"""
    k = 16
    rec = HR.generator_records(4200)                                       # counters up to 67199 > 2^16
    assert len(rec) * k > (1 << 16) + 1000
    cases_ = {}
    for seed, offset, ff in ((7, 0.0, False), (7, 1e-3, True), (0x123456789ABC, 1e-3, False), (0x123456789ABC, 0.0, True)):
        cases_[(seed, offset, ff)] = HR.hemisphere_rays(rec, k, seed, offset, ff)
    return k, rec, cases_


@pytest.mark.parametrize("policy", POLICIES)
def test_rays_are_the_float64_generators(policy, generator_reference):
    k, rec, refs = generator_reference
    t = tracer(workload("c2"), policy)
    try:
        feats = to_device(rec)
        worst_d = worst_o = worst_len = 0.0
        for (seed, offset, ff), (mask, want) in refs.items():
            _, got, _ = hemispheres(t, feats, k, False, True, seed=seed, offset=offset, face_forward=ff)
            _, again, _ = hemispheres(t, feats, k, False, True, seed=seed, offset=offset, face_forward=ff)
            assert got.tobytes() == again.tobytes()                        # deterministic
            assert mask.sum() > 3000 and (~mask).sum() > 300
            assert not got[~mask].view(np.uint8).any()                     # no hemisphere: zero bytes
            assert (got["x"][mask] == np.arange(len(rec), dtype=np.uint32)[mask, None]).all() and (got["y"] == 0).all()
            d = got["d"][mask].astype(np.float64)
            cos = (d * HR.unit_normals(rec, ff)[mask][:, None, :]).sum(-1)
            dev_d = np.abs(d - want["d"][mask]).max()
            dev_o = np.abs(got["o"][mask].astype(np.float64) - want["o"][mask]).max()
            dev_len = np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max()
            print("policy", policy, "seed %#x offset %g ff %d" % (seed, offset, ff), "max |d - ref| %.3g  |o - ref| %.3g  ||d| - 1| %.3g  min cos %.3g"
                  % (dev_d, dev_o, dev_len, cos.min()))
            worst_d, worst_o, worst_len = max(worst_d, dev_d), max(worst_o, dev_o), max(worst_len, dev_len)
            assert cos.min() > 0
            assert dev_d <= RAY_BOUND and dev_o <= RAY_BOUND and dev_len <= RAY_BOUND, (policy, seed, offset, ff)
            if offset == 0.0:                                              # the origin is the point itself
                assert (got["o"][mask] == rec["pos"][mask][:, None, :]).all()
        # the second seed gives other rays, the high key word counts, and so does the face-forward flag where it applies
        a, b = refs[(7, 0.0, False)][1], refs[(0x123456789ABC, 1e-3, False)][1]
        assert np.abs(a["d"] - b["d"]).max() > 0.5
        print("policy", policy, "worst: d %.3g o %.3g len %.3g (bound %.3g)" % (worst_d, worst_o, worst_len, RAY_BOUND))
    finally:
        t.close()


# ---- 4. nothing of the context moves ---------------------------------------------------------------------------------------------
def test_the_calls_move_no_state():
    import torch
    wl = workload("all_kinds")
    t = tracer(wl, 2, OPT_MOMENTS=1)
    lib = R.load_library()
    try:
        fresh = tracer(wl, 2)
        try:                                            # a fresh context has no feature records, before and after
            rec = HR.generator_records()
            counts, _, _ = hemispheres(fresh, to_device(rec), 4, True, True, seed=1, t_max=INF)
            assert len(counts) == len(rec)
            buf = np.empty((H, W), dtype=A.FEATURE)
            assert lib.rt_read_features(fresh._ctx, buf.ctypes.data, buf.nbytes) == ESTATE
            with pytest.raises(R.RtError) as e:         # and its own records cannot be asked about
                fresh.occludedHemispheres(None, 4)
            assert e.value.code == ESTATE
        finally:
            fresh.close()
        feats = to_device(first_hits(t, wl.camera))
        t.clear()
        t.renderSamples(wl.camera, 0, 4)
        t.resolve()
        t.enableCounters(True)

        def state():
            t.sync()
            accum = torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()
            return (accum.tobytes(), t.transferImage().tobytes(), t.sample_counter, t.moments().tobytes(), t.featureRecords().tobytes(),
                    t.counters().as_dict())        # (the values: a Counters object's repr is its address)

        before = state()
        hemispheres(t, feats, 64, True, True, seed=2, offset=1e-3, t_max=2.0, face_forward=True)
        hemispheres(t, None, 5, True, False, seed=2, t_max=INF)
        hemispheres(t, None, 3, False, True, seed=2)
        t.ambientOcclusion(4, 2.0)
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


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    import torch
    wl = workload("c2")
    t = tracer(wl)
    lib = R.load_library()
    try:
        n, k = W * H, 4
        feats = to_device(first_hits(t, wl.camera))
        cnt = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        out = torch.full((n * k, 8), 3.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        fp, cp, rp = (C.c_void_p(x.data_ptr()) for x in (feats, cnt, out))
        P = A.HemisphereParams

        def prefill_holds():
            t.sync()
            torch.cuda.synchronize()
            return bool((cnt == 7).all()) and bool((out == 3.0).all())

        def hemi(ctx, f, m, p, c, r):
            rc = lib.rt_occluded_hemispheres(ctx, f, m, C.byref(p) if p is not None else None, c, r)
            assert rc != 0 and prefill_holds(), ("rt_occluded_hemispheres wrote", m)
            return rc

        good = P(k, 1, 7, 1e-3, INF)
        assert hemi(None, fp, n, good, cp, rp) == EINVAL
        assert hemi(t._ctx, fp, n, None, cp, rp) == EINVAL                                   # no parameters
        assert hemi(t._ctx, fp, n, good, None, None) == EINVAL                               # both outputs NULL
        assert hemi(t._ctx, fp, 0, good, cp, rp) == EINVAL
        assert hemi(t._ctx, fp, (1 << 28) + 1, good, cp, rp) == EINVAL
        assert hemi(t._ctx, fp, n, P(0, 1, 7, 0.0, INF), cp, rp) == EINVAL                   # k 0
        assert hemi(t._ctx, fp, 1, P(A.RAY_SET_MAX + 1, 1, 7, 0.0, INF), cp, rp) == EINVAL
        assert hemi(t._ctx, fp, (1 << 20) + 1, P(2048, 1, 7, 0.0, INF), cp, rp) == EINVAL    # more than 2^31 rays
        assert hemi(t._ctx, C.c_void_p(feats.data_ptr() + 8), n - 1, good, cp, rp) == EINVAL # misaligned pointers
        assert hemi(t._ctx, fp, n, good, C.c_void_p(cnt.data_ptr() + 2), rp) == EINVAL
        assert hemi(t._ctx, fp, n - 1, good, cp, C.c_void_p(out.data_ptr() + 8)) == EINVAL
        assert hemi(t._ctx, fp, n, P(k, 2, 7, 0.0, INF), cp, rp) == EINVAL                   # unknown flag bits
        assert hemi(t._ctx, fp, n, P(k, 0x80000001, 7, 0.0, INF), cp, rp) == EINVAL
        for bad in (INF, -INF, float("nan")):
            assert hemi(t._ctx, fp, n, P(k, 1, 7, bad, INF), cp, rp) == EINVAL               # a non-finite offset
        assert hemi(t._ctx, None, n - 1, good, cp, rp) == EINVAL                             # NULL features with n != W * H
        t.setShard(0, 2, 8, 8)
        assert hemi(t._ctx, fp, n, good, cp, rp) == EINVAL                                   # a sharded context
        with pytest.raises(ValueError):
            t.occludedHemispheres(feats, k, out=cnt)
        t.setShard(0, 1, 8, 8)
        ctx = C.c_void_p()
        assert lib.rt_create(0, W, H, C.byref(ctx)) == 0
        assert hemi(ctx, fp, n, good, cp, rp) == ESTATE                                      # no scene
        lib.rt_destroy(ctx)
        t.resize(W, H)                                                                       # a reallocated frame: no records
        assert hemi(t._ctx, None, n, good, cp, rp) == ESTATE
        for kw in (dict(out=cnt[:-1]), dict(out=cnt.float()), dict(rays_out=out[:-1]), dict(k=0), dict(k=A.RAY_SET_MAX + 1),
                   dict(offset=INF)):
            with pytest.raises(ValueError):
                t.occludedHemispheres(feats, **dict(dict(k=k, out=cnt, rays_out=out), **kw))
        with pytest.raises(ValueError):
            t.spawnHemispheres(feats[:-1], k, out=out)
        assert prefill_holds()
        assert lib.rt_occluded_hemispheres(t._ctx, fp, n, C.byref(good), cp, rp) == 0        # and the same buffers are fine
        t.sync()
        assert int(cnt.max()) <= k and int(cnt.min()) >= 0 and not bool((out == 3.0).all())
    finally:
        t.close()


# ---- 6. ambientOcclusion, the C++ façade and rt_cli --ao K --ao-device -----------------------------------------------------------
def read_pfm(path, w, h):
    raw = open(path, "rb").read()
    head = b"Pf\n%d %d\n-1.0\n" % (w, h)
    assert raw.startswith(head)
    return np.frombuffer(raw, np.float32, w * h, len(head))


def test_ambient_occlusion_and_cli_are_one_minus_count_over_k(built, tmp_path):
    """ambientOcclusion and rt_cli --aov P --ao 8 --ao-device are 1 - counts / 8 of the same rt_occluded_hemispheres call,
    exactly.  Against the host-path picture (plain --ao 8: float64 rays numbered by hit, not by pixel, so other rays of the
    same distribution) the share of differing pixels and the mean difference are printed, not asserted."""
    w, h, k = 96, 54, 8
    scene_file = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    common = [os.path.join(cases.ROOT, "host", "rt_cli"), "--scene", scene_file, "--size", "%dx%d" % (w, h), "--spp", "1",
              "--camera=-8,-1,-8,45,0", "--ao", str(k), "--ao-distance", "4"]
    p = subprocess.run(common + ["--aov", str(tmp_path / "dev"), "--ao-device"], check=True, cwd=cases.ROOT, capture_output=True, text=True)
    assert "ambient occlusion: 8 device-made rays per pixel" in p.stdout
    got = read_pfm(str(tmp_path / "dev_ao.pfm"), w, h)
    subprocess.run(common + ["--aov", str(tmp_path / "host")], check=True, cwd=cases.ROOT, capture_output=True, text=True)
    host = read_pfm(str(tmp_path / "host_ao.pfm"), w, h)
    s = rt.SceneCreator()
    s.loadScene(scene_file, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        cam = rt.Camera(60, F32(w) / F32(h), (-8, -1, -8), 45.0, 0.0)
        t.renderFeatures(cam)
        rec = t.featureRecords().reshape(-1)
        hit = (rec["flags"] & A.FEATURE_HIT) != 0
        counts = t.occludedHemispheres(None, k, seed=0xC0FFEE, offset=0.0, t_max=4.0, face_forward=True)
        ao = t.ambientOcclusion(k, 4.0, seed=0xC0FFEE)
        t.sync()
        counts = counts.cpu().numpy()
        want = F32(1) - counts.astype(F32) / F32(k)
        assert tuple(ao.shape) == (h, w) and str(ao.dtype) == "torch.float32"
        assert np.array_equal(ao.cpu().numpy().reshape(-1), want)
        assert np.array_equal(got, want)
        assert hit.any() and (~hit).any() and 0 < counts.sum() < hit.sum() * k and (want[~hit] == 1).all()
        print("device-made against host-made rays: %.1f %% of the pixels differ, mean AO %.4f against %.4f"
              % (100.0 * (got != host).mean(), got.mean(), host.mean()))
    finally:
        t.close()
