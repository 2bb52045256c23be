"""GPU (-m gpu): the hemisphere gather, rt_render_hemispheres.  What the call adds to its target is, bit for bit and in all
four channels, what rt_render_ray_sets adds over the very rays the spawn form of rt_occluded_hemispheres writes — under every
policy and RT_OPT_ACCEL, in every kernel family, for records without a hemisphere at the edges of a wave's slots and for a
whole wave of them; such records keep their bytes; nothing else of the context moves; a refused call writes nothing;
irradiance() and rt_cli --gather are pi * rgb / count of the same call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import hemisphere_ref as HR
import moments_ref as M

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
R = rt.raytracer
T = rt.RayTracer
F32 = np.float32
EINVAL, ESTATE = -1, -4
FIXED, QUEUE = A.CAMERA_PLAN_FIXED, A.CAMERA_PLAN_QUEUE
W, H = 48, 27
POLICIES = [0, 1, 2]
SCENES = {
    "c2": dict(),
    "all_kinds": dict(),
    "c4": dict(n_spheres=3000),               # a sphere BVH
    "c5": dict(segments=24, rings=16),        # a mesh BVH
}
POISON = 0xDEADBEEF
KW = dict(seed=11, offset=1e-3, face_forward=True)


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
    t.renderFeatures(camera)
    return t.featureRecords().reshape(-1).copy()


def knock_out(rec, every=7):
    """Every `every`-th record loses its hemisphere, by turns the hit flag and the normal → the records, the valid mask"""
    rec = rec.copy()
    idx = np.arange(len(rec))
    rec["flags"][idx % (2 * every) == 3] = 0
    rec["normal"][idx % (2 * every) == 3 + every] = 0
    return rec, HR.valid_mask(rec)


def start_target(n, mask, seed=1):
    """What a target holds before a call: random finite sums and counts on the records that have a hemisphere (so that
    'adds' is visible), poison on the others (so that 'untouched' is) → (n, 4) float32 on the host"""
    rs = np.random.RandomState(seed)
    init = (rs.rand(n, 4) * 4).astype(F32)
    init[:, 3] = rs.randint(0, 9, n)
    init[~mask] = np.uint32(POISON).view(F32)
    return init


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return d


def gathered(t, feats, k, first, count, init, **kw):
    """renderHemispheres into a copy of `init` → (n, 4) float32 on the host"""
    out = on_device(init)
    assert t.renderHemispheres(feats, k, first, count, out=out, **dict(KW, **kw)) is out
    t.sync()
    return out.cpu().numpy()


def twin(t, feats, k, first, count, init, **kw):
    """The two calls the gather replaces, into another copy of `init`: spawnHemispheres, then renderRaySets over its rays →
    (n, 4) float32 on the host, and the rays on the device"""
    out = on_device(init)
    rays = t.spawnHemispheres(feats, k, **dict(KW, **kw))
    t.renderRaySets(rays, k, first, count, out=out)
    t.sync()
    return out.cpu().numpy(), rays


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_contract(t, feats, mask, k, first, count, tag, **kw):
    """gather == twin in bytes on the valid records; the others keep their bytes; the counts grew by `count` → the gather's
    result and what it started from"""
    n = len(mask)
    init = start_target(n, mask)
    got = gathered(t, feats, k, first, count, init, **kw)
    want, _ = twin(t, feats, k, first, count, init, **kw)
    assert same_bits(got[mask], want[mask]), (tag, np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1) & mask)[:10])
    assert same_bits(got[~mask], init[~mask]), (tag, "a record without a hemisphere was written")
    assert (got[mask, 3] == init[mask, 3] + count).all(), tag
    return got, init


# ---- 1. the exact contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_gather_adds_what_the_ray_sets_of_the_spawned_rays_add(name, policy, accel):
    wl = workload(name)
    t = tracer(wl, policy, OPT_ACCEL=accel)
    try:
        rec, mask = knock_out(first_hits(t, wl.camera))
        assert mask.any() and (~mask).any()
        feats = to_device(rec)
        lit = False
        for k in (1, 5, 64, 100):
            for first, count in ((0, k), (3, 2 * k + 3)):
                # (k = 5: a seed whose two words are NaN patterns as floats — the key travels in FrameParams::cam)
                got, init = check_contract(t, feats, mask, k, first, count, (name, policy, accel, k, first, count),
                                           seed=0x7FA00000FFC12345 if k == 5 else k)
                moved = (got[mask, :3] != init[mask, :3]).any(1)
                print(name, policy, accel, "k", k, "samples", first, count, "valid", int(mask.sum()), "records that received radiance", int(moved.sum()))
                lit |= bool(moved.any())
                assert t.lastRayPlan()[1]["family"] == QUEUE
        assert lit                                                        # some valid record received radiance
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 2. shapes where the run logic can break -----------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [0, 2])
@pytest.mark.parametrize("name", ["all_kinds", "c4"])
def test_invalid_records_at_the_edges_of_a_waves_slots_and_a_whole_wave_of_them(name, policy):
    import torch
    wl = workload(name)
    t = tracer(wl, policy)
    try:
        base = first_hits(t, wl.camera)
        base = base[HR.valid_mask(base)]                                  # the test places the invalid records itself
        k, first, count = 5, 3, 13
        n = len(base)
        assert n >= 400
        # what a wave owns, from a first call over the same number of records and samples
        gathered(t, to_device(base), k, first, count, np.zeros((n, 4), F32))
        facts, plan = t.lastRayPlan()
        ppw = plan["pixels_per_wave"]
        assert plan["family"] == QUEUE and facts["n"] == n and 1 <= ppw <= 64
        if n % ppw == 0:
            n -= 1
            base = base[:n]
        waves = np.arange((n + ppw - 1) // ppw)
        assert len(waves) >= 6
        bad = np.zeros(n, bool)
        bad[ppw * waves[waves % 3 == 0]] = True                           # the first slot of some waves
        bad[np.minimum(ppw * waves[waves % 3 == 1] + ppw - 1, n - 1)] = True   # the last slot of others
        bad[ppw * 3:ppw * 4] = True                                       # a whole wave: it leaves before staging
        bad[5::11] = True
        rec = base.copy()
        rec["flags"][bad & (np.arange(n) % 2 == 0)] = 0                   # some lack only the hit flag,
        rec["normal"][bad & (np.arange(n) % 2 == 1)] = 0                  # some have a zero normal
        mask = HR.valid_mask(rec)
        assert np.array_equal(mask, ~bad) and n % ppw != 0
        feats = to_device(rec)
        check_contract(t, feats, mask, k, first, count, (name, policy, "edges"))
        assert t.lastRayPlan()[1]["pixels_per_wave"] == ppw and t.lastRayPlan()[0]["n"] == n
        # two launches, 512 + 88 samples, over one record and over seventy
        for m in (1, 70):
            lo = max(ppw * 3 - 35, 0)                                        # (seventy records around the wave without any)
            sub = np.flatnonzero(mask)[:1] if m == 1 else np.arange(lo, lo + 70)
            assert len(sub) == m and mask[sub].any() and (m == 1 or (~mask[sub]).any())
            check_contract(t, to_device(rec[sub]), mask[sub], k, 0, 600, (name, policy, "600 samples", m))
        # against the plain per-ray call, sample by sample, summed on the host: independent of the set logic
        zeros = np.zeros((n, 4), F32)
        got = gathered(t, feats, k, first, count, zeros)
        _, rays = twin(t, feats, k, first, count, zeros)
        pick = np.concatenate([np.flatnonzero(mask)[[0, 1, -1]], np.flatnonzero(mask & (np.arange(n) // ppw == 2))[-2:],
                               np.flatnonzero(mask & (np.arange(n) // ppw == 4))[:2]])
        sums = np.zeros((len(pick), 3))
        sets = rays.view(n, k, 8)
        index = torch.from_numpy(pick).cuda()
        for s in range(first, first + count):
            one = torch.zeros((len(pick), 4), dtype=torch.float32, device="cuda")
            batch = sets[index, s % k].contiguous()
            torch.cuda.synchronize()
            t.renderRays(batch, s, 1, out=one)
            t.sync()
            one = one.cpu().numpy()
            assert (one[:, 3] == 1).all()
            sums += one[:, :3].astype(np.float64)
        mine = got[pick, :3].astype(np.float64)
        print(name, policy, "per-sample sums, max relative deviation", float((np.abs(mine - sums) / np.maximum(sums, 1e-30)).max()))
        assert (np.abs(mine - sums) <= 1e-6 * sums).all() and sums.any() and (got[pick, 3] == count).all()
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 3. every kernel family gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["c2", "c5"])
def test_every_kernel_family_gives_the_same_bits(name, policy):
    wl = workload(name)
    k, first, count = 8, 3, 24
    t = tracer(wl, policy)
    try:
        rec, mask = knock_out(first_hits(t, wl.camera))
        feats, n = to_device(rec), len(rec)
        want, init = check_contract(t, feats, mask, k, first, count, (name, policy, "queue"))
        assert t.lastRayPlan()[1]["family"] == QUEUE
        t.setOption(T.OPT_SAMPLE_QUEUE, 0)
        assert same_bits(gathered(t, feats, k, first, count, init), want) and t.lastRayPlan()[1]["family"] == FIXED
        t.setOption(T.OPT_SAMPLE_QUEUE, 1)
        t.enableCounters(True)
        t.resetCounters()
        assert same_bits(gathered(t, feats, k, first, count, init), want)
        _, plan = t.lastRayPlan()
        assert plan["family"] == FIXED and plan["count"] == 1
        every = t.counters().as_dict()
        # the counters: rt_render_ray_sets' over the valid sets alone — the invalid records removed from both inputs
        kept = to_device(rec[mask])
        start = np.zeros((int(mask.sum()), 4), F32)
        t.resetCounters()
        mine_out = gathered(t, kept, k, first, count, start)
        mine = t.counters().as_dict()
        t.resetCounters()
        theirs_out, _ = twin(t, kept, k, first, count, start)
        theirs = t.counters().as_dict()
        assert same_bits(mine_out, theirs_out)
        assert mine == theirs and mine["samples"] == int(mask.sum()) * count and mine["bounces"] > 0
        assert every["samples"] == int(mask.sum()) * count                 # the invalid records add nothing to the counters
        t.enableCounters(False)
        t.close()
        lanes = 32                                                         # (24 samples: 32 lanes per record)
        for options in (dict(OPT_MAX_THREADS_PER_LAUNCH=n * lanes // 3 + 64), dict(OPT_MAX_THREADS_PER_LAUNCH=n * lanes // 3 + 64, OPT_SAMPLE_QUEUE=0),
                        dict(OPT_WAVE_FILL=0), dict(OPT_WAVE_FILL=1)):
            t = tracer(wl, policy, **options)
            assert same_bits(gathered(t, feats, k, first, count, init), want), options
            facts, plan = t.lastRayPlan()
            if "OPT_MAX_THREADS_PER_LAUNCH" in options:
                per = (n * lanes // 3 + 64) // lanes
                assert facts["n"] == n - 2 * per and 0 < facts["n"] <= per, "the last of three slot ranges"
            assert plan["family"] == (FIXED if "OPT_SAMPLE_QUEUE" in options else QUEUE)
            assert t.walkOverflow() == 0
            t.close()
    finally:
        t.close()


# ---- 4. the accumulator as the target, and the moments -----------------------------------------------------------------------
def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().reshape(-1, 4).copy()


@pytest.mark.parametrize("policy", POLICIES)
def test_accumulator_target_resolve_denoise_and_moments(policy):
    wl = workload("all_kinds")
    k = 8
    t = tracer(wl, policy)
    try:
        rec = first_hits(t, wl.camera)
        mask = HR.valid_mask(rec)
        assert mask.any() and (~mask).any()                               # the frame has misses of its own
        ext = gathered(t, None, k, 0, k, np.zeros((W * H, 4), F32))
        t.clear()
        assert t.renderHemispheres(None, k, **KW) is None                 # n_samples None: k; into the accumulator
        acc = read_accum(t)
        assert same_bits(acc, ext) and not acc[~mask].any() and (acc[mask, 3] == k).all() and acc[mask, :3].any()
        t.resolve()
        image = t.transferImage()
        assert np.isfinite(image).all() and image[..., :3].any()
        assert np.isfinite(t.denoise()).all() and np.isfinite(t.denoiseVariance()).all()
        # moments: from a frame with samples everywhere, so that "updated as rt_render_ray_sets" and "untouched" both show
        t.setOption(T.OPT_MOMENTS, 1)
        results = []
        for which in ("gather", "twin"):
            t.clear()
            t.renderSamples(wl.camera, 0, 4)
            before = (read_accum(t), t.moments().reshape(-1).copy())
            if which == "gather":
                t.renderHemispheres(None, k, 2, 2 * k + 1, **KW)
            else:
                t.renderRaySets(t.spawnHemispheres(None, k, **KW), k, 2, 2 * k + 1)
            facts, plan = t.lastRayPlan()
            assert plan["family"] == FIXED and plan["moments"] == 1
            results.append((before, read_accum(t), t.moments().reshape(-1).copy()))
        (b0, a0, m0), (b1, a1, m1) = results
        assert same_bits(b0[0], b1[0]) and same_bits(b0[1], b1[1]) and b0[1].any()
        assert same_bits(a0[mask], a1[mask]) and same_bits(a0[~mask], b0[0][~mask])
        assert same_bits(m0[~mask], b0[1][~mask])                          # untouched where there is no hemisphere
        assert not same_bits(m0[mask], b0[1][mask])
        # on the valid pixels: the twin's, to the tolerance of the moments tests (tests/moments_ref.py tolerance: the largest
        # sample luminance is bounded by the sum of them, radiance being non-negative)
        n_total = a1[mask, 3].astype(np.float64)
        lum_sum = a1[mask, :3].astype(np.float64) @ M.LUM
        tol = M.tolerance(m1[mask], n_total, lum_sum)
        err = np.abs(m0[mask].astype(np.float64) - m1[mask])
        print("policy", policy, "moments: max |gather - twin| %.3g (largest tolerance %.3g), bits equal: %s" % (err.max(), tol.max(), same_bits(m0[mask], m1[mask])))
        assert (err <= tol).all() and (m0 >= 0).all()
        assert np.isfinite(t.denoiseMoments()).all()
        # an external target keeps no moments
        ext_before = t.moments().copy()
        gathered(t, None, k, 0, k, np.zeros((W * H, 4), F32))
        assert same_bits(t.moments(), ext_before)
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 5. nothing else moves -----------------------------------------------------------------------------------------------------
def test_the_call_moves_no_state():
    import torch
    wl = workload("all_kinds")
    t = tracer(wl, 2, OPT_MOMENTS=1)
    lib = R.load_library()
    try:
        fresh = tracer(wl, 2)
        try:                                            # a fresh context has no feature records, before and after
            rec = HR.generator_records()
            out = gathered(fresh, to_device(rec), 4, 0, 4, np.zeros((len(rec), 4), F32))
            assert (out[:, 3] == 4 * HR.valid_mask(rec)).all()
            buf = np.empty((H, W), dtype=A.FEATURE)
            assert lib.rt_read_features(fresh._ctx, buf.ctypes.data, buf.nbytes) == ESTATE
            with pytest.raises(R.RtError) as e:         # and its own records cannot be gathered from
                fresh.renderHemispheres(None, 4)
            assert e.value.code == ESTATE
        finally:
            fresh.close()
        feats = to_device(first_hits(t, wl.camera))
        t.clear()
        t.renderSamples(wl.camera, 0, 4)
        t.resolve()

        def state():
            t.sync()
            accum = torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()
            return (accum.tobytes(), t.transferImage().tobytes(), t.sample_counter, t.moments().tobytes(), t.featureRecords().tobytes(),
                    t.counters().as_dict())

        before = state()
        zeros = np.zeros((W * H, 4), F32)
        gathered(t, feats, 64, 0, 64, zeros)
        gathered(t, None, 5, 7, 600, zeros)
        t.irradiance(4, 2)
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


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    import torch
    wl = workload("c2")
    t = tracer(wl)
    lib = R.load_library()
    try:
        n, k = W * H, 4
        feats = to_device(first_hits(t, wl.camera))
        out = torch.full((n, 4), 3.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        fp, op = C.c_void_p(feats.data_ptr()), C.c_void_p(out.data_ptr())
        P = A.HemisphereParams
        INF = float("inf")
        t.clear()
        accum0 = read_accum(t)

        def prefill_holds():
            t.sync()
            torch.cuda.synchronize()
            return bool((out == 3.0).all()) and same_bits(read_accum(t), accum0)

        def gather(ctx, f, m, p, first, count, o):
            rc = lib.rt_render_hemispheres(ctx, f, m, C.byref(p) if p is not None else None, first, count, o)
            assert rc != 0 and prefill_holds(), ("rt_render_hemispheres wrote", m, first, count)
            return rc

        good = P(k, 1, 7, 1e-3, INF)
        assert gather(None, fp, n, good, 0, k, op) == EINVAL
        assert gather(t._ctx, fp, n, None, 0, k, op) == EINVAL                                # no parameters
        assert gather(t._ctx, fp, 0, good, 0, k, op) == EINVAL
        assert gather(t._ctx, fp, (1 << 28) + 1, good, 0, k, op) == EINVAL
        assert gather(t._ctx, fp, n, P(0, 1, 7, 0.0, INF), 0, k, op) == EINVAL                # k 0
        assert gather(t._ctx, fp, 1, P(A.RAY_SET_MAX + 1, 1, 7, 0.0, INF), 0, k, op) == EINVAL
        assert gather(t._ctx, fp, (1 << 20) + 1, P(2048, 1, 7, 0.0, INF), 0, k, op) == EINVAL # more than 2^31 rays
        assert gather(t._ctx, C.c_void_p(feats.data_ptr() + 8), n - 1, good, 0, k, op) == EINVAL   # misaligned pointers
        assert gather(t._ctx, fp, n - 1, good, 0, k, C.c_void_p(out.data_ptr() + 8)) == EINVAL
        assert gather(t._ctx, fp, n, P(k, 2, 7, 0.0, INF), 0, k, op) == EINVAL                # unknown flag bits
        assert gather(t._ctx, fp, n, P(k, 0x80000001, 7, 0.0, INF), 0, k, op) == EINVAL
        for bad in (INF, -INF, float("nan")):
            assert gather(t._ctx, fp, n, P(k, 1, 7, bad, INF), 0, k, op) == EINVAL            # a non-finite offset
        assert gather(t._ctx, fp, n, good, 0, 0, op) == EINVAL                                # no samples
        assert gather(t._ctx, fp, n, good, A.MAX_SAMPLE, 2, op) == EINVAL                     # samples beyond RT_MAX_SAMPLE
        assert gather(t._ctx, fp, n, good, 1, A.MAX_SAMPLE + 1, op) == EINVAL
        assert gather(t._ctx, None, n - 1, good, 0, k, op) == EINVAL                          # NULL features with n != W * H
        assert gather(t._ctx, fp, n - 1, good, 0, k, None) == EINVAL                          # NULL target with n != W * H
        t.setShard(0, 2, 8, 8)
        accum0 = read_accum(t)
        assert gather(t._ctx, fp, n, good, 0, k, op) == EINVAL                                # a sharded context
        with pytest.raises(ValueError):
            t.renderHemispheres(feats, k, out=out)
        t.setShard(0, 1, 8, 8)
        accum0 = read_accum(t)
        ctx = C.c_void_p()
        assert lib.rt_create(0, W, H, C.byref(ctx)) == 0
        assert gather(ctx, fp, n, good, 0, k, op) == ESTATE                                   # no scene
        lib.rt_destroy(ctx)
        t.resize(W, H)                                                                        # a reallocated frame: no records
        accum0 = read_accum(t)
        assert gather(t._ctx, None, n, good, 0, k, op) == ESTATE
        assert gather(t._ctx, None, n, good, 0, k, None) == ESTATE
        for kw in (dict(out=out[:-1]), dict(out=out.double()), dict(out=out[:, :3]), dict(k=0), dict(k=A.RAY_SET_MAX + 1), dict(offset=INF),
                   dict(n_samples=0), dict(first_sample=A.MAX_SAMPLE, n_samples=2)):
            with pytest.raises(ValueError):
                t.renderHemispheres(feats, **dict(dict(k=k, out=out), **kw))
        with pytest.raises(ValueError):
            t.renderHemispheres(feats[:-1], k)                                                # the accumulator takes W * H records
        assert prefill_holds()
        assert lib.rt_render_hemispheres(t._ctx, fp, n, C.byref(good), 0, k, op) == 0        # and the same buffers are fine
        t.sync()
        got = out.cpu().numpy()
        mask = HR.valid_mask(A.feature_records(feats))
        assert (got[mask, 3] == 3.0 + k).all() and (got[~mask] == 3.0).all() and (got[mask, :3] != 3.0).any()
        t.clear()
        assert lib.rt_render_hemispheres(t._ctx, fp, n, C.byref(good), k, 600, None) == 0    # ... and the accumulator
        acc = read_accum(t)
        assert (acc[mask, 3] == 600).all() and not acc[~mask].any()
    finally:
        t.close()


# ---- 7. irradiance() and rt_cli --gather K ------------------------------------------------------------------------------------
def read_pfm3(path, w, h):
    raw = open(path, "rb").read()
    head = b"PF\n%d %d\n-1.0\n" % (w, h)
    assert raw.startswith(head) and len(raw) == len(head) + 12 * w * h
    return np.frombuffer(raw, np.float32, 3 * w * h, len(head)).reshape(h * w, 3)


def test_irradiance_and_cli_are_pi_times_the_mean_of_the_same_call(built, tmp_path):
    w, h, k, each = 96, 54, 8, 3
    scene_file = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    common = [os.path.join(cases.ROOT, "host", "rt_cli"), "--scene", scene_file, "--size", "%dx%d" % (w, h), "--spp", "1",
              "--camera=-8,-1,-8,45,0"]
    p = subprocess.run(common + ["--aov", str(tmp_path / "one"), "--gather", str(k)], check=True, cwd=cases.ROOT, capture_output=True, text=True)
    assert "irradiance: 8 device-made directions per pixel, 1 samples each" in p.stdout
    p = subprocess.run(common + ["--aov", str(tmp_path / "three"), "--gather", str(k), "--gather-spp", str(each)], check=True, cwd=cases.ROOT,
                       capture_output=True, text=True)
    assert "irradiance: 8 device-made directions per pixel, 3 samples each" in p.stdout
    s = rt.SceneCreator()
    s.loadScene(scene_file, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        cam = rt.Camera(60, F32(w) / F32(h), (-8, -1, -8), 45.0, 0.0)
        t.renderFeatures(cam)
        rec = t.featureRecords().reshape(-1)
        hit = (rec["flags"] & A.FEATURE_HIT) != 0
        for spp, prefix in ((1, "one"), (each, "three")):
            acc = gathered(t, None, k, 0, k * spp, np.zeros((w * h, 4), F32), seed=0xC0FFEE, offset=1e-3, face_forward=True)
            assert (acc[hit, 3] == k * spp).all() and not acc[~hit].any()
            want = np.zeros((w * h, 3), F32)
            want[hit] = (F32(np.pi) * acc[hit, :3]) / acc[hit, 3:4]          # binary32: one product, one quotient
            e = t.irradiance(k, spp, seed=0xC0FFEE)
            t.sync()
            assert tuple(e.shape) == (h, w, 3) and str(e.dtype) == "torch.float32" and e.device.type == "cuda"
            assert same_bits(e.cpu().numpy().reshape(-1, 3), want)
            assert same_bits(read_pfm3(str(tmp_path / (prefix + "_irradiance.pfm")), w, h), want)
            assert want[hit].any() and not want[~hit].any()
            print("irradiance, %d samples per direction: mean %.4f over the hits, %.1f %% of the pixels hit" % (spp, want[hit].mean(), 100 * hit.mean()))
    finally:
        t.close()
