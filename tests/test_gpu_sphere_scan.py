"""GPU (-m gpu): the brute-force sphere scan that asks the wave first (csrc/pt_device.hpp sphere_take<FAST>,
PT_SPHERE_ANY_FIRST: `if (__any(dis > 0))` in front of the per-lane test; DESIGN §5 and §8, profiles/r30_experiments.md),
which the sample-queue kernels without counters and without a BVH walk run under policies 1 and 2.  Everything is compared
as uint32 with ==, under policies 0, 1 and 2 (policy 0 has no tagged scan: its kernels are the parent's byte for byte).

1. Crafted rays.  Scene: five spheres of C2's materials and the unit sphere at (1, 0, 5), no plane.  Per sphere the classes
   a lane can be in — misses the line; front hit; sphere behind the origin with the origin outside (b < 0, cc > 0), near and
   with |b| > 1024; origin inside; origin on the surface (the hit point of a query, outgoing and incoming directions) — and
   on the unit sphere the tangent whose discriminant is exactly 0 in float32 with its neighbours one ulp of b either side,
   and b = +0 and b = -0 from outside and from inside.  The classes are checked with intersectRays, an independent kernel,
   and are not empty.  A fresh lane of the ray kernels goes straight into the nearest-hit search with the caller's origin
   and direction, and the same call with OPT_SAMPLE_QUEUE 0 runs the fixed-lane kernel, which keeps the untagged scan.
   * renderRaySets, sets of 4 and 4 samples, reaches pt_samples_q_raysets<false, 0, 6> and puts 64 different records on the
     64 lanes of a wave (16 sets a wave, lane l = record l).  Waves: every lane of one class; exactly one lane of another
     class at lane 0, 31, 32 and 63; classes alternating; seeded random mixtures; a wave of 36 lanes — the smallest shapes at
     which a wrong mask nesting or a wrong uniform branch shows.
   * renderRays reaches pt_samples_q_rays<false, 0, 6>, where a wave owns 16 rays at 1 sample (lanes 0 .. 15, the rest idle)
     and 13 or 16 at 5 samples (five lanes a ray; RT_OPT_WAVE_FILL 1 or 0): the same compositions per group of 16 resp. 13
     rays — waves that are mostly idle lanes, and runs of five equal lanes.
   Both launches' plans are read back and pixels_per_wave is asserted, so the groups are the waves.
2. Frames of the fused path (pt_prefix + pt_samples_q) against the direct path pt_render as tests/test_gpu_mixcol.py
   compares them: C2 and C3 at 61 x 37 and 7 x 5, counts (spp, first) = (1, 0), (5, 3), (64, 0), (200, 7), and C2 seen from
   inside its glass sphere.  The CPU oracle lights a good part of each frame, so none of them is black."""
import numpy as np
import pytest

import cases
from oracle import Oracle

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
T = rt.RayTracer
f32 = np.float32
WAVE = 64
POLICIES = [0, 1, 2]
UNIT = 5   # index of the unit sphere at (1, 0, 5)


def _scene():
    s = rt.SceneCreator()
    for typ, col, extra in ((A.T_REFLECTIVE, (1, 1, 1), 0.85), (A.T_REFRACTIVE, (1, 1, 1), 1.5), (A.T_DIFFUSE, (0.9, 0.15, 0.1), 1.0),
                            (A.T_DIELECTRIC, (0.8, 0.9, 1), 1.6), (A.T_LIGHT, (1, 1, 1), 0.0), (A.T_DIFFUSE, (0.15, 0.85, 0.35), 1.0)):
        s.addMaterial(typ, col, extra)
    s.addSphere((-6.0, 0.5, 12.0), 2.0, 0)       # mirror
    s.addSphere((6.0, 3.25, 14.0), 1.75, 1)      # glass
    s.addSphere((-7.0, -4.0, 3.0), 1.0, 2)       # red diffuse
    s.addSphere((8.0, -3.0, 4.5), 2.5, 3)        # tinted crystal
    s.addSphere((1.0, -200.0, 0.0), 100.0, 4)    # the light overhead (world up is -y)
    s.addSphere((1.0, 0.0, 5.0), 1.0, 5)         # the unit sphere of the tangent rays
    return s


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def _perp(d):
    a = np.where(np.abs(d[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])
    return _unit(np.cross(d, a))


def _class_rays(scene, rng):
    """{class: (origins (n, 3), directions (n, 3), sphere index (n,))} — without the two surface classes, which need a query."""
    c = scene.spheres["pos"][:, :3].astype(np.float64)
    r = scene.spheres["r"].astype(np.float64)
    out = {k: ([], [], []) for k in ("miss", "front", "behind_near", "behind_far", "inside")}

    def put(k, o, d, i):
        out[k][0].append(np.asarray(o, f32)); out[k][1].append(np.asarray(d, f32)); out[k][2].append(i)

    for i in range(len(c)):
        for _ in range(6):
            u = _unit(rng.normal(size=(1, 3)))[0].astype(np.float64)          # from the centre towards the origin
            p = _perp(u[None])[0].astype(np.float64)
            o = c[i] + u * (r[i] + 1.0 + 3.0 * rng.random())
            put("front", o, _unit(c[i] + p * r[i] * 0.6 * rng.random() - o), i)
            dist = np.linalg.norm(o - c[i])                                   # r + 1 .. r + 4, at least 1.01 r
            put("miss", o, _unit(p + 0.16 * (rng.random() - 0.5) * u), i)     # across: the line passes at 0.996 dist or more
            put("behind_near", o, _unit(u + 0.5 * rng.random() * r[i] / dist * p), i)   # the sphere behind, on the line
            of = c[i] + u * (r[i] + 1500.0 + 500.0 * rng.random())
            put("behind_far", of, _unit(u + 1e-4 * rng.random() * p), i)             # ... and |b| > 1024
            put("inside", c[i] + u * r[i] * 0.7 * rng.random(), _unit(rng.normal(size=3)), i)
    return {k: (np.array(o, f32), np.array(d, f32), np.array(i)) for k, (o, d, i) in out.items()}


def _edge_rays():
    """On the unit sphere at (1, 0, 5): the tangent with dis == 0 exactly — oc = (1, 0, 5), b = 5, cc = 26 - 1, dis = 25 - 25 — and
    its neighbours with b one ulp above (dis = b * b - 25 is 2.5 or 3 ulps of 25: a hit near t = 5) and one below (dis < 0);
    b = +0 and -0 (every product of the dot is a zero of that sign) from outside and inside."""
    ulp = f32(2.0 ** -21)                                                             # of b = 5
    tang_o = np.zeros((3, 3), f32)
    tang_d = np.array([[0, 0, 1], [ulp, 0, 1], [-ulp, 0, 1]], f32)                    # b = 5, 5 + ulp, 5 - ulp; cc = 25
    assert (f32(1) * tang_d[:, 0] + f32(5) == np.array([5, np.nextafter(f32(5), f32(6)), np.nextafter(f32(5), f32(4))], f32)).all()
    zero_o = np.array([[1, 0, -3], [1, 0, -3], [1, 0, 5.5], [1, 0, 5.5]], f32)          # oc = (0, 0, 8) and (0, 0, -0.5)
    zero_d = np.array([[1, 0, 0], [-1, -0.0, -0.0], [1, 0, 0], [-1, -0.0, 0.0]], f32)
    return {"tangent": (tang_o, tang_d, np.full(3, UNIT)), "b_zero": (zero_o, zero_d, np.full(4, UNIT))}


def _query(t, o, d):
    import torch
    batch = rt.rays.pack_rays(o, d)
    out = t.intersectRays(torch.from_numpy(rt.rays.as_floats(batch).copy()).cuda())
    t.sync()
    return A.feature_records(out)


def _on_sphere(rec, idx):
    return ((rec["flags"] & A.FEATURE_HIT) != 0) & (rec["object"] == (idx.astype(np.uint32)))   # K_SPHERE = 0 << 30


def _classes(t, scene):
    """The classes, checked with the query kernel under the tracer's policy.  → {class: (origins, directions)}"""
    cl = _class_rays(scene, np.random.default_rng(30))
    cl.update(_edge_rays())
    hit = {k: _on_sphere(_query(t, o, d), i) for k, (o, d, i) in cl.items()}
    assert hit["front"].all() and hit["inside"].all()
    assert not hit["miss"].any() and not hit["behind_near"].any() and not hit["behind_far"].any()
    assert list(hit["tangent"]) == [False, True, False], hit["tangent"]          # dis == 0 is no hit; one ulp inside is
    assert list(hit["b_zero"]) == [False, False, True, True], hit["b_zero"]
    # origins on the surface: the hit points of the front rays, leaving along the normal and entering against it
    o, d, i = cl["front"]
    rec = _query(t, o, d)
    pos, nrm = rec["pos"].astype(f32), rec["normal"].astype(f32)
    bend = _perp(nrm) * f32(0.3)
    cl["surface_out"] = (pos, _unit(nrm + bend), i)
    cl["surface_in"] = (pos, _unit(-nrm + bend), i)
    # what the scan sees of each class: b < 0 with cc > 0 behind, cc < 0 inside, |b| > 1024 far behind
    c, r = scene.spheres["pos"][:, :3], scene.spheres["r"]
    for k, (o, d, i) in cl.items():
        assert len(o) >= 3 and o.dtype == f32 and d.dtype == f32, k
        oc = (c[i] - o).astype(np.float64)
        b, cc = (oc * d).sum(1), (oc * oc).sum(1) - r[i].astype(np.float64) ** 2
        if k.startswith("behind"):
            assert (b < 0).all() and (cc > 0).all() and (b * b - cc > 0).all(), k
            assert (np.abs(b) > 1024).all() if k == "behind_far" else (np.abs(b) < 1024).all(), k
        if k == "inside":
            assert (cc < 0).all()
        if k == "miss":
            assert (b * b - cc < 0).all()
        if k.startswith("surface"):
            assert (np.abs(cc) < 1e-3 * r[i] ** 2).all() and ((b < 0) if k == "surface_out" else (b > 0)).all(), k
    return {k: (o, d) for k, (o, d, _) in cl.items()}


def _groups(cl, g, short):
    """The batch as groups of g rays — g is what ONE WAVE takes in its first refill, lane by lane — and a last group of
    `short` rays: every lane of one class; exactly one lane of another class at the group's first lane, either side of its
    middle (lanes 31 and 32 of a full wave: the two halves the 32-wide SIMD issues one after the other) and its last lane;
    classes alternating lane by lane; seeded mixtures of all classes.  → (origins, directions, number of groups)"""
    rng = np.random.default_rng(31)
    names = sorted(cl)

    def take(k, n, start=0):
        o, d = cl[k]
        j = (start + np.arange(n)) % len(o)
        return o[j], d[j]

    groups = []
    for k in names:                                           # every lane of one class
        groups.append(take(k, g))
    pairs = (("miss", "front"), ("behind_near", "inside"), ("front", "miss"), ("behind_far", "surface_out"), ("miss", "tangent"))
    for n, (base, other) in enumerate(pairs):                  # exactly one lane of another class
        for lane in (0, g // 2 - 1, g // 2, g - 1):
            o, d = take(base, g, lane)
            o, d = o.copy(), d.copy()
            o[lane], d[lane] = (x[0] for x in take(other, 1, lane + n))
            groups.append((o, d))
    for a, b in (("miss", "front"), ("behind_near", "surface_in"), ("b_zero", "tangent")):   # alternating, lane by lane
        oa, da = take(a, g); ob, db = take(b, g)
        even = (np.arange(g) % 2 == 0)[:, None]
        groups.append((np.where(even, oa, ob), np.where(even, da, db)))
    for _ in range(3):                                        # a seeded mixture of all classes
        picks = [take(names[rng.integers(len(names))], 1, int(rng.integers(1000))) for _ in range(g)]
        groups.append((np.concatenate([p[0] for p in picks]), np.concatenate([p[1] for p in picks])))
    o, d = groups[-1]
    assert 0 < short < g
    groups.append((o[:short][::-1].copy(), d[:short][::-1].copy()))   # a wave that is not full
    return np.concatenate([w[0] for w in groups]), np.concatenate([w[1] for w in groups]), len(groups)


def _both_scans(t, launch, n_out, spp, policy, what, pixels_per_wave):
    """launch(out) through the sample queue (the tagged scan) and with OPT_SAMPLE_QUEUE 0 (the fixed-lane kernel, which keeps
    the untagged scan) → the two (n_out, 4) results; `pixels_per_wave`: what the QUEUE launch's plan must show."""
    import torch
    outs = []
    for queue, family in ((1, A.CAMERA_PLAN_QUEUE), (0, A.CAMERA_PLAN_FIXED)):
        t.setOption(T.OPT_SAMPLE_QUEUE, queue)
        out = torch.zeros((n_out, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        launch(out)
        t.sync()
        facts, plan = t.lastRayPlan()
        assert (plan["family"], plan["accel"], plan["geom"]) == (family, 0, 0), (policy, what, plan)
        assert facts["count_enabled"] == 0 and facts["n"] == n_out and facts["count"] == spp, (policy, what, facts)
        if queue:
            assert plan["pixels_per_wave"] == pixels_per_wave, (policy, what, plan)
        outs.append(out.cpu().numpy())
    return outs


def _assert_same(outs, spp, policy, what):
    tagged, untagged = (x.view(np.uint32) for x in outs)
    assert (untagged[:, 3] == f32(spp).view(np.uint32)).all()
    lit = float((outs[1][:, :3] > 0).any(axis=1).mean())
    print("policy %d, %s: %.3f of the %d results carry light" % (policy, what, lit, len(tagged)))
    assert lit >= 0.02, lit                                # (a black batch would compare equal whatever the code does)
    bad = (tagged != untagged).any(axis=1)
    assert not bad.any(), (policy, what, int(bad.sum()), np.flatnonzero(bad)[:8], outs[0][bad][:4], outs[1][bad][:4])


def _device_rays(o, d):
    import torch
    return torch.from_numpy(rt.rays.as_floats(rt.rays.pack_rays(o, d)).copy()).cuda()


SET = 4   # records per ray set = samples per ray: 16 rays x 4 samples are the 64 lanes of a wave, each with a record of its own


@pytest.mark.parametrize("policy", POLICIES)
def test_crafted_ray_sets_put_64_rays_on_the_64_lanes_of_a_wave(policy):
    """pt_samples_q_raysets<false, 0, 6>: a wave owns pixels_per_wave = 16 ray sets (QUEUE_MAX_PIXELS); with 4 samples through
    sets of 4 its queue holds 64 entries, all taken in the first refill — lane l starts at entry l, which is sample l % 4 of
    set l / 4 of the wave, i.e. record l of the wave's 64 consecutive records.  The groups of 64 ARE the waves' lanes."""
    scene = _scene()
    assert len(scene.planes) == 0 and len(scene.spheres) == 6
    t = T(16, 16, scene=scene, seed=cases.SEED)
    t.setArith(policy)
    t.setOption(T.OPT_WAVE_FILL, 1)   # (the default; tests/conftest.py gives a test either value by its name — 16 sets a wave both ways)
    try:
        o, d, n_waves = _groups(_classes(t, scene), WAVE, 36)
        assert len(o) == (n_waves - 1) * WAVE + 36 and len(o) % SET == 0 and len(o) < 4000
        n_sets = len(o) // SET
        assert WAVE // SET == 16 and -(-n_sets // 16) == n_waves        # 16 sets a wave: wave w holds records 64 w .. 64 w + 63
        rays = _device_rays(o, d)
        outs = _both_scans(t, lambda out: t.renderRaySets(rays, SET, 0, SET, out=out), n_sets, SET, policy, "ray sets", 16)
        _assert_same(outs, SET, policy, "%d records in %d waves of 64 lanes" % (len(o), n_waves))
        assert t.walkOverflow() == 0
    finally:
        t.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_crafted_rays_through_the_tagged_scan_equal_the_untagged_scan(policy):
    """pt_samples_q_rays<false, 0, 6>: a wave owns pixels_per_wave consecutive rays — 16 at 1 sample (QUEUE_MAX_PIXELS: lanes
    0 .. 15 start at one ray each, the other 48 stay idle); at 5 samples, five lanes a ray, 13 under RT_OPT_WAVE_FILL 1
    (ceil(64 / 5): the 65th entry goes to the first lane that retires) and 16 under RT_OPT_WAVE_FILL 0 (80 entries, 64 of
    them in the first refill).  The option is set here — tests/conftest.py gives a test either value by its name — and the
    groups are laid out by pixels_per_wave, which is read back from the launch's plan and asserted."""
    scene = _scene()
    t = T(16, 16, scene=scene, seed=cases.SEED)
    t.setArith(policy)
    try:
        cl = _classes(t, scene)
        for spp, fill, g in ((1, 1, 16), (5, 1, 13), (5, 0, 16)):
            t.setOption(T.OPT_WAVE_FILL, fill)
            o, d, n_waves = _groups(cl, g, g // 2 + 1)
            n = len(o)
            assert n == (n_waves - 1) * g + g // 2 + 1
            rays = _device_rays(o, d)
            outs = _both_scans(t, lambda out: t.renderRays(rays, 0, spp, out=out), n, spp, policy, "%d spp, wave fill %d" % (spp, fill), g)
            _assert_same(outs, spp, policy, "%d rays in %d waves of %d rays, %d spp, wave fill %d" % (n, n_waves, g, spp, fill))
        assert t.walkOverflow() == 0
    finally:
        t.close()


# ---- 2. frames --------------------------------------------------------------------------------------------------------------
COUNTS = ((1, 0), (5, 3), (64, 0), (200, 7))   # (spp, first)
SIZES = {"ragged": (61, 37), "tiny": (7, 5)}
GLASS_CENTRE = (0.0, 3.2, -0.5)                # C2's refractive sphere, r = 1.8 (assets/scenes/c2_cornell.scene)


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


FRAMES = [("c2", "ragged"), ("c2", "tiny"), ("c3", "ragged"), ("c3", "tiny"), ("c2_inside_glass", "ragged")]
GEOM = {"c2": 0, "c3": 1, "c2_inside_glass": 0}


@pytest.fixture(scope="module")
def lit_by_the_oracle():
    """Fraction of the pixels the CPU oracle lights with 4 samples, per frame of FRAMES — computed once."""
    out = {}
    t = T(8, 8, scene=rt.workloads.get("c1", width=8, height=8).scene, seed=cases.SEED)   # (the table of the seed every tracer here uses)
    try:
        table = t.getRandomTable()
    finally:
        t.close()
    orc = Oracle()
    for case, size in FRAMES:
        wl = _workload(case, size)
        img, _ = orc.render(wl.scene, wl.camera, table, wl.width, wl.height, 2, count=4, threads=4)
        out[case, size] = float((img[..., :3] > 0).any(axis=2).mean())
    print("lit fractions by the CPU oracle:", out)
    return out


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("case,size", FRAMES)
def test_fused_frames_equal_the_direct_path(case, size, policy, lit_by_the_oracle):
    assert lit_by_the_oracle[case, size] >= 0.1, lit_by_the_oracle      # not a black frame
    wl = _workload(case, size)
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    t.setArith(policy)
    try:
        for spp, first in COUNTS:
            frames = []
            for share, queue in ((1, 1), (0, 0)):   # fused path with the sample queue; direct path pt_render
                t.setOption(t.OPT_PREFIX_SHARING, share)
                t.setOption(t.OPT_SAMPLE_QUEUE, queue)
                t.clear()
                t.renderSamples(wl.camera, first, spp)
                t.sync()
                frames.append(t.readLinear().copy())
                if share:   # the queue family ran, without counters and without a BVH walk
                    facts, plan = t.lastSamplePlan()
                    assert plan["family"] == A.PLAN_QUEUE and facts["count_enabled"] == 0, (case, policy, spp, facts, plan)
                    assert plan["geom"] == GEOM[case] and plan["accel"] == 0, (case, policy, spp, plan)
                    if spp == 64:
                        assert plan["count_log2"] == 6, (case, policy, plan)
            fused, direct = frames
            assert (direct[..., :3] > 0).any(), (case, size, policy, spp)
            same = fused.view(np.uint32) == direct.view(np.uint32)
            assert same.all(), (case, size, policy, spp, first, int((~same).any(axis=2).sum()))
        assert t.walkOverflow() == 0
    finally:
        t.close()
