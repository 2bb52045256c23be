"""CPU: which sample kernel a fused launch runs, with how many pixels per wave, how much LDS and how many workgroups —
plan_samples of csrc/pt_kernels.hip through rt_debug_plan_samples (the launcher calls the same function), against its
Python restatement (tests/sample_plan_ref.py) over the cross product of everything the choice reads, and against a handful
of rows written out by hand so that the restatement cannot drift together with the code.  Every sample kernel returns the
same bits, so nothing else notices a launch that picked a slower instantiation."""
import itertools

import pytest

import cases
import sample_plan_ref as R

rt = cases.rt
plan_samples = rt.raytracer.plan_samples
FIXED, QUEUE, WALK, GENERIC = R.FIXED, R.QUEUE, R.WALK, R.GENERIC

# (lenses, models, faces, spheres, sphere BVH, mesh BVH, walk jobs); 6 materials and one plane throughout
GEOMETRY = {
    "spheres": (0, 0, 0, 8, 0, 0, 0),
    "lens": (1, 0, 0, 8, 0, 0, 0),
    "small_mesh_12": (0, 1, 12, 8, 0, 0, 0),
    "small_meshes_65": (0, 2, 65, 8, 0, 0, 0),
    "sphere_bvh": (0, 0, 0, 2000, 1, 0, 0),
    "sphere_bvh_lens": (1, 0, 0, 2000, 1, 0, 0),
    "bvh_mesh": (0, 1, 1000, 8, 0, 1, 1),
    "bvh_meshes_2": (0, 2, 2000, 8, 0, 1, 2),
    "bvh_mesh_small_mesh": (0, 2, 1012, 8, 0, 1, 0),
}
COUNTS = [(c, R.group_log2_for(c)) for c in (1, 8, 63, 64, 65, 384, 512, 513)] + [(64, 5)]


def _facts(geometry, count, glog2, n, counters, moments, queue, walk, fill, exact):
    lenses, models, faces, spheres, sphere_bvh, mesh_bvh, jobs = GEOMETRY[geometry]
    seg_cap = -(-n // 256) * 256
    light, heavy = {"unknown": (0, 0), "known": (n // 3, n // 7), "none_live": (0, 0)}[exact]
    return dict(count=count, glog2=glog2, n=n, seg_cap=seg_cap, material_count=6, sphere_count=spheres, plane_count=1,
                lens_count=lenses, model_count=models, sphere_bvh=sphere_bvh, mesh_bvh=mesh_bvh, walk_jobs=jobs, faces=faces,
                cu_count=256, count_enabled=counters, sample_queue=queue, walk_slices=walk, wave_fill=fill, moments=moments,
                exact=int(exact != "unknown"), count_light=light, count_heavy=heavy)


@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_the_plan_equals_its_restatement(built, geometry):
    families = set()
    for (count, glog2), n, exact in itertools.product(COUNTS, (256, 2073600), ("unknown", "known", "none_live")):
        for counters, moments, queue, walk, fill in itertools.product((0, 1), repeat=5):
            f = _facts(geometry, count, glog2, n, counters, moments, queue, walk, fill, exact)
            got, want = plan_samples(**f), R.plan(f)
            assert got == want, (f, got, want)
            families.add(got["family"])
            # what every plan must satisfy, whatever the rules: a queue fits its wave, and no live pixel means no launch
            if got["family"] != FIXED:
                assert 1 <= got["pixels_per_wave"] <= 16 and got["pixels_per_wave"] * count <= max(512, count)
                assert got["block_size"] == 64 and got["lds_bytes"] <= 65536
            assert (got["grid_units"] == 0) == (exact == "none_live")
    assert FIXED in families and QUEUE in families and (WALK in families) == (GEOMETRY[geometry][6] != 0)


def test_a_chip_of_unknown_size_counts_as_256_compute_units(built):
    f = _facts("spheres", 64, 6, 200 * 126, 0, 0, 1, 1, 1, "unknown")
    assert plan_samples(**dict(f, cu_count=0)) == plan_samples(**f) == R.plan(f)
    # 25 200 pixels over 16 x 4 x 6 x 16 = 6 144 wanted waves: 4 pixels each; over 256 x 384: one (64 samples fill the lanes)
    assert plan_samples(**dict(f, cu_count=16))["pixels_per_wave"] == 4 and plan_samples(**f)["pixels_per_wave"] == 1


def test_refuses_facts_no_launch_can_have(built):
    f = _facts("spheres", 64, 6, 256, 0, 0, 1, 1, 1, "unknown")
    for bad in (dict(count=0), dict(glog2=7), dict(seg_cap=0)):
        with pytest.raises(rt.RtError):
            plan_samples(**dict(f, **bad))


# ---- rows written out by hand ---------------------------------------------------------------------------------------------
HD = 1920 * 1080


def _scene(name, **kw):
    return rt.workloads.get(name, width=16, height=16, **kw).scene


def _key(p):
    log2 = -1 if p["count_log2"] == GENERIC else p["count_log2"]
    return (p["family"], bool(p["count"]), bool(p["accel"]), p["geom"], p["waves"], bool(p["moments"]), log2)


def test_c2_at_1080p_and_64_samples(built):
    c2 = _scene("c2")
    p = plan_samples(**R.facts_of(c2, HD, 64))
    assert _key(p) == (QUEUE, False, False, 0, 6, False, 6)
    static = 2 * len(c2.materials) + 2 * len(c2.spheres) + len(c2.planes)
    assert (p["pixels_per_wave"], p["grid_units"], p["block_size"]) == (6, HD // 6 + 1, 64)
    assert p["lds_bytes"] == 16 * static + 6 * (6 * 16 + 64 * 12) and p["lds_face_f4"] == 0
    # moments and counters keep the generic kernel; so does a launch of 64 samples on 32 lanes per pixel
    assert _key(plan_samples(**R.facts_of(c2, HD, 64, moments=1))) == (QUEUE, False, False, 0, 6, True, -1)
    assert _key(plan_samples(**R.facts_of(c2, HD, 64, count_enabled=1))) == (QUEUE, True, False, 0, 6, False, -1)
    assert _key(plan_samples(**R.facts_of(c2, HD, 64, glog2=5))) == (QUEUE, False, False, 0, 6, False, -1)
    for other in (dict(moments=1), dict(count_enabled=1), dict(glog2=5)):
        q = plan_samples(**R.facts_of(c2, HD, 64, **other))
        assert (q["pixels_per_wave"], q["grid_units"], q["lds_bytes"]) == (6, HD // 6 + 1, p["lds_bytes"])


def test_c2_small_frames_spread_over_the_chip(built):
    c2 = _scene("c2")
    p = plan_samples(**R.facts_of(c2, 200 * 126, 64))
    assert _key(p) == (QUEUE, False, False, 0, 6, False, 6) and p["pixels_per_wave"] == 1 and p["grid_units"] == 25344 + 1
    assert plan_samples(**R.facts_of(c2, 200 * 126, 64, wave_fill=0))["pixels_per_wave"] == 6
    # a resting camera whose live list is known: exactly the waves that own a pixel
    p = plan_samples(**R.facts_of(c2, 200 * 126, 64, exact=1, count_light=1000, count_heavy=10))
    assert p["grid_units"] == 1010
    assert plan_samples(**R.facts_of(c2, 200 * 126, 64, exact=1))["grid_units"] == 0


def test_c3_stages_its_cube_in_lds_without_losing_a_pixel(built):
    c3 = _scene("c3", tex_size=8)
    static = 2 * len(c3.materials) + 2 * len(c3.spheres) + len(c3.planes)
    for count in (64, 256):
        p = plan_samples(**R.facts_of(c3, HD, count))
        assert _key(p)[:5] == (QUEUE, False, False, 1, 6) and p["lds_face_f4"] == 36
        assert p["pixels_per_wave"] == rt.raytracer.queue_pixels(count, 6, static) == rt.raytracer.queue_pixels(count, 6, static + 36)
        assert p["lds_bytes"] == 16 * (static + 36) + p["pixels_per_wave"] * (6 * 16 + count * 12)
    assert plan_samples(**R.facts_of(c3, HD, 64, count_enabled=1))["lds_face_f4"] == 0   # a counting launch scans global memory
    assert _key(plan_samples(**R.facts_of(c3, HD, 64))) == (QUEUE, False, False, 1, 6, False, 6)


def test_c4_runs_the_sphere_bvh_kernel(built):
    c4 = _scene("c4", n_spheres=2000)
    for moments in (0, 1):
        p = plan_samples(**R.facts_of(c4, HD, 64, moments=moments))
        assert _key(p) == (QUEUE, False, True, 0, R.D["PT_Q_WAVES_SPHERE_BVH"], bool(moments), -1)
    assert R.D["PT_Q_WAVES_SPHERE_BVH"] == 6 and R.D["PT_Q_WAVES_ACCEL"] == 5
    assert _key(plan_samples(**R.facts_of(c4, HD, 64, accel=0))) == (QUEUE, False, False, 0, 6, False, 6)   # brute force
    # a lens beside the spheres: the general geometry code needs the registers of 5 waves per SIMD
    assert _key(plan_samples(**dict(R.facts_of(c4, HD, 64), lens_count=1))) == (QUEUE, False, True, 1, 5, False, -1)


def test_c5_walks_in_slices(built):
    c5 = _scene("c5", segments=16, rings=10)
    f = R.facts_of(c5, HD, 64)
    assert (f["mesh_bvh"], f["walk_jobs"], f["faces"]) == (1, 1, 2 * 16 * 9)
    p = plan_samples(**f)
    assert (p["family"], p["multi"], p["moments"], p["waves"]) == (WALK, 0, 0, R.D["PT_W_WAVES"])
    assert plan_samples(**dict(f, moments=1))["moments"] == 1 and plan_samples(**dict(f, walk_jobs=2))["multi"] == 1
    assert plan_samples(**dict(f, walk_jobs=2))["waves"] == R.D["PT_W_WAVES_MULTI"] == 4
    assert _key(plan_samples(**dict(f, walk_slices=0))) == (QUEUE, False, True, 2, 5, False, -1)
    assert _key(plan_samples(**dict(f, count_enabled=1))) == (QUEUE, True, True, 2, 5, False, -1)
    assert _key(plan_samples(**R.facts_of(c5, HD, 64, accel=0))) == (QUEUE, False, False, 1, 6, False, 6)   # the face scan


def test_more_samples_than_a_queue_holds_run_the_fixed_lane_kernel(built):
    c2 = _scene("c2")
    p = plan_samples(**R.facts_of(c2, HD, 513))
    assert (p["family"], p["count"], p["accel"], p["pixels_per_wave"], p["block_size"], p["lds_bytes"]) == (FIXED, 0, 0, 1, 256, 0)
    assert p["grid_units"] == ((HD + 1) * 64 + 255) // 256
    assert plan_samples(**R.facts_of(c2, HD, 512))["family"] == QUEUE
    assert plan_samples(**R.facts_of(c2, HD, 64, sample_queue=0))["family"] == FIXED
