"""Host restatement of the camera launcher's plan (csrc/pt_kernels.hip plan_camera_samples) and of the facts it is made
from (csrc/rt_context.hpp camera_facts), for tests/test_cameras_host.py and tests/test_gpu_cameras.py."""
import cases
import sample_plan_ref as S
from test_wave_fixed_host import pixels_per_wave

rt = cases.rt
A = rt._abi
D = S.D
FIXED, QUEUE = A.CAMERA_PLAN_FIXED, A.CAMERA_PLAN_QUEUE
group_log2_for = S.group_log2_for


def plan(f):
    """plan_camera_samples, rule by rule in the order the launcher applies them: facts (dict) → plan (dict)."""
    count = f["count"]
    queue = bool(f["sample_queue"]) and count <= D["QUEUE_SLOTS"] and not f["count_enabled"] and not f["moments"]
    accel = bool(f["sphere_bvh"] or f["mesh_bvh"])
    simple_geom = not f["lens_count"] and not f["model_count"]
    sphere_bvh_only = bool(f["sphere_bvh"]) and not f["mesh_bvh"]
    p = dict(family=FIXED, count=int(bool(f["count_enabled"])), accel=int(accel), geom=0, waves=0, moments=int(bool(f["moments"])),
             pixels_per_wave=1, lds_face_f4=0, lds_bytes=0, grid_units=((f["n"] << f["glog2"]) + 255) // 256, block_size=256)
    if not queue:
        return p
    geom = (0 if simple_geom else 1) if (not accel or sphere_bvh_only) else 2
    waves = D["PT_Q_WAVES"] if not accel else (D["PT_Q_WAVES_SPHERE_BVH"] if sphere_bvh_only and simple_geom else D["PT_Q_WAVES_ACCEL"])
    static_f4 = A.stage_block_layout(f["material_count"], f["sphere_count"], f["plane_count"])[3]
    ppw_of = lambda static: pixels_per_wave(count, waves, static, D["PT_LDS_GRANULE"], D["QUEUE_SLOTS"], D["QUEUE_MAX_PIXELS"])
    want_units = (f["cu_count"] or 256) * 4 * 6 * D["PT_UNITS_PER_WAVE_SLOT"]
    ppw_par = max(f["n"] // want_units, -(-64 // count)) if f["wave_fill"] else D["QUEUE_MAX_PIXELS"]
    ppw = min(ppw_of(static_f4), ppw_par)
    nf = f["faces"]
    face_f4 = 0
    if D["PT_FACE_MASK"] and not simple_geom and not f["mesh_bvh"] and 0 < nf <= D["PT_LDS_FACE_CAP"] and ppw_of(static_f4 + 3 * nf) >= ppw:
        face_f4 = 3 * nf
        static_f4 += face_f4
    p.update(family=QUEUE, geom=geom, waves=waves, pixels_per_wave=ppw, lds_face_f4=face_f4, block_size=64,
             grid_units=-(-f["n"] // ppw), lds_bytes=16 * static_f4 + ((ppw * (96 + 12 * count) + 15) & ~15))
    return p


def facts_of(scene, n, count, **options):
    """camera_facts for a slot range of `n` slots of `scene` under the options of sample_plan_ref.facts_of."""
    f = S.facts_of(scene, n, count, **options)
    return {k: f[k] for k, _ in A.CameraFacts._fields_}
