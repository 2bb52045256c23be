"""Host restatement of the fused launcher's sample-kernel plan (csrc/pt_kernels.hip plan_samples) and of the facts it is
made from (csrc/rt_context.hpp sample_facts), for tests/test_sample_plan_host.py and tests/test_gpu_sample_plan.py."""
import os
import re

import cases
from test_wave_fixed_host import pixels_per_wave

rt = cases.rt
A = rt._abi
CSRC = os.path.join(cases.ROOT, "opencl-raytracing_amd", "csrc")
FIXED, QUEUE, WALK = A.PLAN_FIXED, A.PLAN_QUEUE, A.PLAN_WALK
GENERIC = A.PLAN_GENERIC_COUNT


def _defines():
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("pt_kernels.hip", "pt_device.hpp", "rt_context.hpp"))
    names = ("QUEUE_SLOTS", "QUEUE_MAX_PIXELS", "PT_Q_WAVES", "PT_Q_WAVES_ACCEL", "PT_Q_WAVES_SPHERE_BVH", "PT_W_WAVES",
             "PT_W_WAVES_MULTI", "PT_UNITS_PER_WAVE_SLOT", "PT_LDS_FACE_CAP", "PT_LDS_GRANULE", "PT_Q_COUNT64", "PT_FACE_MASK",
             "ACCEL_MIN_SPHERES", "MESH_BVH_MIN_FACES")
    return {n: int(re.search(r"#define\s+%s\s+(\d+)" % n, text).group(1)) for n in names}


D = _defines()


def group_log2_for(count):
    g = 0
    while (1 << g) < count and g < 6:
        g += 1
    return g


def sample_units(seg_cap, per_unit, light, heavy):
    """rt_sample_units (tests/test_sample_grid_host.py pins it against live_take)"""
    cnt_l = min(light, seg_cap)
    cnt_h = min(heavy, seg_cap - cnt_l)
    return -(-cnt_h // per_unit) + -(-cnt_l // per_unit)


def plan(f):
    """plan_samples, rule by rule in the order the launcher applies them: facts (dict) → plan (dict)."""
    count = f["count"]
    queue = bool(f["sample_queue"]) and count <= D["QUEUE_SLOTS"]
    accel = bool(f["sphere_bvh"] or f["mesh_bvh"])
    simple_geom = not f["lens_count"] and not f["model_count"]
    sphere_bvh_only = bool(f["sphere_bvh"]) and not f["mesh_bvh"]
    q_waves = D["PT_Q_WAVES"] if not accel else (D["PT_Q_WAVES_SPHERE_BVH"] if sphere_bvh_only and simple_geom else D["PT_Q_WAVES_ACCEL"])
    static_f4 = A.stage_block_layout(f["material_count"], f["sphere_count"], f["plane_count"])[3]
    ppw_of = lambda waves, static: pixels_per_wave(count, waves, static, D["PT_LDS_GRANULE"], D["QUEUE_SLOTS"], D["QUEUE_MAX_PIXELS"])
    want_units = (f["cu_count"] or 256) * 4 * 6 * D["PT_UNITS_PER_WAVE_SLOT"]
    ppw_par = max(f["n"] // want_units, -(-64 // count)) if f["wave_fill"] else D["QUEUE_MAX_PIXELS"]
    ppw = min(ppw_of(q_waves, static_f4), ppw_par)
    face_f4 = 0
    nf = f["faces"]
    if (D["PT_FACE_MASK"] and not simple_geom and not f["mesh_bvh"] and not f["count_enabled"] and 0 < nf <= D["PT_LDS_FACE_CAP"]
            and ppw_of(q_waves, static_f4 + 3 * nf) >= ppw):
        face_f4 = 3 * nf
        static_f4 += face_f4
    p = dict(family=FIXED, count=int(bool(f["count_enabled"])), accel=int(accel), geom=0, waves=0, moments=int(bool(f["moments"])),
             count_log2=0, multi=0, lds_face_f4=face_f4, lds_bytes=0, block_size=64)
    if queue and f["mesh_bvh"] and f["walk_jobs"] and f["walk_slices"] and not f["count_enabled"]:
        p.update(family=WALK, multi=int(f["walk_jobs"] != 1))
        p["waves"] = D["PT_W_WAVES_MULTI"] if p["multi"] else D["PT_W_WAVES"]
        ppw = min(ppw_of(p["waves"], static_f4), ppw_par)
    elif queue:
        if not accel:
            geom = 0 if simple_geom else 1
        elif sphere_bvh_only:
            geom = 0 if simple_geom else 1
        else:
            geom = 2
        count64 = bool(D["PT_Q_COUNT64"]) and not accel and not p["count"] and not p["moments"] and count == 64 and f["glog2"] == 6
        p.update(family=QUEUE, geom=geom, waves=q_waves, count_log2=6 if count64 else GENERIC)
    else:
        p["block_size"] = 256
        ppw = 1
    units = -(-f["seg_cap"] // ppw) + 1
    if f["exact"]:
        units = sample_units(f["seg_cap"], ppw, f["count_light"], f["count_heavy"])
    p["pixels_per_wave"] = ppw
    if p["family"] == FIXED:
        p["grid_units"] = ((units << f["glog2"]) + 255) // 256
    else:
        p["grid_units"] = units
        p["lds_bytes"] = 16 * static_f4 + ((ppw * (96 + 12 * count) + 15) & ~15)
    return p


def facts_of(scene, n, count, glog2=None, accel=1, cu_count=256, count_enabled=0, sample_queue=1, walk_slices=1, wave_fill=1,
             moments=0, exact=0, count_light=0, count_heavy=0):
    """sample_facts for a slot range of `n` slots of `scene` (a SceneCreator) under the given options (accel: RT_OPT_ACCEL)."""
    faces = [int(v) for v in scene.meshes["face_count"]]
    has_bvh = [v >= D["MESH_BVH_MIN_FACES"] for v in faces]
    jobs = [m["mesh_anchor"] + k for m in scene.models for k in range(m["mesh_count"])]
    all_bvh = any(has_bvh) and len(scene.models) > 0 and all(j < len(faces) and has_bvh[j] for j in jobs)
    ns = len(scene.spheres)
    return dict(count=count, glog2=group_log2_for(count) if glog2 is None else glog2, n=n, seg_cap=-(-n // 256) * 256,
                material_count=len(scene.materials), sphere_count=ns, plane_count=len(scene.planes),
                lens_count=len(scene.lenses), model_count=len(scene.models),
                sphere_bvh=int(ns > 0 and (accel == 2 or (accel == 1 and ns >= D["ACCEL_MIN_SPHERES"]))),
                mesh_bvh=int(accel != 0 and any(has_bvh)), walk_jobs=len(jobs) if all_bvh and jobs else 0, faces=sum(faces),
                cu_count=cu_count, count_enabled=count_enabled, sample_queue=sample_queue, walk_slices=walk_slices,
                wave_fill=wave_fill, moments=moments, exact=exact, count_light=count_light, count_heavy=count_heavy)
