"""ctypes / numpy mirror of include/rt_amd.h (the C ABI of librt_amd.so).

Layouts are the reference's device structs (kernels/raytracer.cl:25-91,
include/scene.h:32-81); sizes are asserted at import.
"""
import ctypes as C

import numpy as np

RT_ABI_VERSION = 3
DEPTH = 30
RANDOM_BUFFER_SIZE = 100000
RANDOM_TABLE_FLOATS = 4 * RANDOM_BUFFER_SIZE
MAX_DIM = 16384
MAX_SAMPLE = 65535

# enum MatType, kernels/raytracer.cl:23
T_REFRACTIVE, T_REFLECTIVE, T_DIELECTRIC, T_DIFFUSE, T_TEXTURED, T_LIGHT = range(6)
MAT_NAMES = {
    "refractive": T_REFRACTIVE,
    "reflective": T_REFLECTIVE,
    "dielectric": T_DIELECTRIC,
    "diffuse": T_DIFFUSE,
    "textured": T_TEXTURED,
    "light": T_LIGHT,
}

MATERIAL = np.dtype([("type", "<i4"), ("_p0", "<i4", (3,)), ("color", "<f4", (4,)), ("extra_data", "<f4"),
                     ("_p1", "<i4", (3,))])
SPHERE = np.dtype([("pos", "<f4", (4,)), ("r", "<f4"), ("mat_ID", "<u4"), ("_p", "<u4", (2,))])
PLANE = np.dtype([("pos", "<f4", (4,)), ("normal", "<f4", (4,)), ("mat_ID", "<u4"), ("_p", "<u4", (3,))])
LENS = np.dtype([("pos", "<f4", (4,)), ("p1", "<f4", (4,)), ("p2", "<f4", (4,)), ("r1", "<f4"), ("r2", "<f4"),
                 ("mat_ID", "<u4"), ("_p", "<u4")])
MESH = np.dtype([("vertex_anchor", "<u4"), ("index_anchor", "<u4"), ("face_count", "<u4"), ("texture_ID", "<u4")])
MODEL = np.dtype([("mesh_anchor", "<u4"), ("mesh_count", "<u4"), ("mat_ID", "<u4")])
assert (MATERIAL.itemsize, SPHERE.itemsize, PLANE.itemsize, LENS.itemsize, MESH.itemsize, MODEL.itemsize) == \
    (48, 32, 48, 64, 16, 12)


class SceneDesc(C.Structure):
    """rt_scene_desc"""
    _fields_ = [(n, C.c_void_p) for n in ("materials", "spheres", "planes", "lenses", "vertices", "uvs", "indices",
                                          "meshes", "models")] + \
               [(n, C.c_uint32) for n in ("material_count", "sphere_count", "plane_count", "lens_count",
                                          "vertex_count", "uv_count", "index_count", "mesh_count", "model_count",
                                          "_pad")]


COUNTER_FIELDS = ("samples", "bounces", "t_sphere", "t_plane", "t_lens", "t_model", "t_mesh", "t_tri", "h_tri",
                  "h_bounce", "n_scatter", "n_dielectric", "n_texfetch", "image_reads")


class Counters(C.Structure):
    """rt_counters"""
    _fields_ = [(n, C.c_uint64) for n in COUNTER_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_FIELDS}

    def algorithmic_bytes(self):
        """SURVEY §8d B_alg: the reference kernel's logical global-memory traffic."""
        c = self
        return (32 * c.t_sphere + 48 * c.t_plane + 64 * c.t_lens + 12 * c.t_model + 16 * c.t_mesh + 60 * c.t_tri +
                36 * c.h_tri + 48 * c.h_bounce + 12 * c.n_scatter + 4 * c.n_dielectric + 64 * c.n_texfetch +
                64 * c.samples + 16 * c.image_reads)


class AdaptiveParams(C.Structure):
    """rt_adaptive_params"""
    _fields_ = [("batch", C.c_uint32), ("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("threshold", C.c_float),
                ("block_w", C.c_uint32), ("block_h", C.c_uint32)]


ADAPTIVE_STATS_FIELDS = ("rounds", "pixel_samples", "blocks", "blocks_at_max")


class AdaptiveStats(C.Structure):
    """rt_adaptive_stats"""
    _fields_ = [("rounds", C.c_uint32), ("pixel_samples", C.c_uint64), ("blocks", C.c_uint32),
                ("blocks_at_max", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in ADAPTIVE_STATS_FIELDS}


def adaptive_prototypes(lib):
    """ctypes prototypes of the adaptive-sampling entry points (rt_render_adaptive & co.)."""
    vp, sz = C.c_void_p, C.c_size_t
    lib.rt_render_adaptive.argtypes = [vp, vp, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStats)]
    lib.rt_read_sample_counts.argtypes = [vp, vp, sz]
    lib.rt_read_block_error.argtypes = [vp, vp, sz]
    lib.rt_render_adaptive_cameras.argtypes = [vp, vp, C.c_uint32, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStats)]
    lib.rt_render_adaptive_variance.argtypes = [vp, vp, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStats)]
    lib.rt_render_adaptive_variance_cameras.argtypes = [vp, vp, C.c_uint32, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStats)]
    lib.rt_read_pixel_error.argtypes = [vp, vp, sz]
    lib.rt_device_pixel_error.argtypes = [vp, C.POINTER(vp)]


def block_error_reference(accum, half, block_w, block_h):
    """Host restatement of the adaptive stopping rule's block error (rt_amd.h, rt_render_adaptive): `accum` and `half`
    are H x W x 4 float32 linear sums (RGB, sample count) of all samples and of the even rounds' samples.  Per pixel,
    in float32 and in the device's order, I = accum / count, A = half / count,
    e = ((|I.r-A.r| + |I.g-A.g|) + |I.b-A.b|) / sqrt((I.r+I.g)+I.b), 0 where the root is 0 or the pixel has no samples;
    per block the mean e over its in-frame pixels (in float64).  → ceil(H/bh) x ceil(W/bw) float64 array."""
    accum = np.asarray(accum, dtype=np.float32)
    half = np.asarray(half, dtype=np.float32)
    h, w = accum.shape[:2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        i = accum[..., :3] / accum[..., 3:4]
        a = half[..., :3] / half[..., 3:4]
        d = np.abs(i - a)
        num = (d[..., 0] + d[..., 1]) + d[..., 2]
        den = np.sqrt((i[..., 0] + i[..., 1]) + i[..., 2])
        ok = den > 0
        e = np.where(ok, num / np.where(ok, den, np.float32(1)), np.float32(0)).astype(np.float64)
    by, bx = -(-h // block_h), -(-w // block_w)
    pad = np.full((by * block_h, bx * block_w), np.nan)
    pad[:h, :w] = e
    return np.nanmean(pad.reshape(by, block_h, bx, block_w), axis=(1, 3))


# rt_feature (rt_render_features): one first-hit record per pixel, 80 bytes in five 16-byte groups
FEATURE = np.dtype([("pos", "<f4", (3,)), ("t", "<f4"), ("normal", "<f4", (3,)), ("object", "<u4"),
                    ("albedo", "<f4", (3,)), ("material", "<u4"), ("dir", "<f4", (3,)), ("face", "<u4"),
                    ("u", "<f4"), ("v", "<f4"), ("tex", "<u4"), ("flags", "<u4")])
assert FEATURE.itemsize == 80
FEATURE_HIT = 1
FEATURE_CUT = 2             # rt_render_features_chain: the terminal has a followed type, max_chain was reached
FEATURE_MIXED = 4           # rt_render_features_cameras: the pixel's samples fall into more than one (object, chain) group
FEATURE_CAMERAS_MAX = 64    # RT_FEATURE_CAMERAS_MAX: camera blocks of one rt_render_features_cameras call
FOLLOW_REFLECTIVE, FOLLOW_REFRACTIVE, FOLLOW_DIELECTRIC = 1, 2, 4   # RT_FOLLOW_*
FOLLOW_NAMES = {"mirror": FOLLOW_REFLECTIVE, "glass": FOLLOW_REFRACTIVE, "dielectric": FOLLOW_DIELECTRIC}
FEATURE_CHAIN_MAX = 29
NO_ID = 0xFFFFFFFF          # object / material / face of a miss; face of a hit that is not a mesh's
OBJECT_KINDS = ("sphere", "plane", "lens", "mesh")   # object id >> 30
DENOISE_SPLIT_OBJECTS = 1
DENOISE_SPLIT_CHAINS = 4
DENOISE_MAX_ITERATIONS = 8
# rt_denoise defaults of the Python and C++ surfaces (DESIGN.md "Feature buffers and denoising": the sweep that chose them)
DENOISE_DEFAULTS = dict(iterations=5, sigma_color=0.5, sigma_normal=0.1, sigma_position=2.0, sigma_albedo=0.2,
                        split_objects=True)


def denoise_flags(split_objects, split_chains=False):
    """rt_denoise_params.flags of the Python surfaces' two switches."""
    return (DENOISE_SPLIT_OBJECTS if split_objects else 0) | (DENOISE_SPLIT_CHAINS if split_chains else 0)


class FeatureChainParams(C.Structure):
    """rt_feature_chain_params"""
    _fields_ = [("follow", C.c_uint32), ("max_chain", C.c_uint32)]


class DenoiseParams(C.Structure):
    """rt_denoise_params"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float), ("sigma_albedo", C.c_float), ("flags", C.c_uint32)]


# rt_denoise_variance defaults of the Python and C++ surfaces (sigma_luminance 4 is SVGF's; DESIGN.md "Variance-guided
# filter")
DENOISE_VARIANCE_EPS = 1e-4
DENOISE_VARIANCE_DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.1, sigma_position=2.0,
                                 sigma_albedo=0.2, split_objects=True)


class DenoiseVarianceParams(C.Structure):
    """rt_denoise_variance_params"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float), ("sigma_albedo", C.c_float), ("flags", C.c_uint32)]


def denoise_prototypes(lib):
    """ctypes prototypes of the feature-buffer and denoiser entry points (rt_render_features & co.)."""
    vp, sz = C.c_void_p, C.c_size_t
    lib.rt_render_features.argtypes = [vp, vp]
    lib.rt_read_features.argtypes = [vp, vp, sz]
    lib.rt_device_features.argtypes = [vp, C.POINTER(vp)]
    lib.rt_denoise.argtypes = [vp, C.POINTER(DenoiseParams)]
    lib.rt_read_denoised.argtypes = [vp, vp, sz]
    lib.rt_device_denoised.argtypes = [vp, C.POINTER(vp)]
    lib.rt_denoise_variance.argtypes = [vp, C.POINTER(DenoiseVarianceParams)]
    lib.rt_read_variance.argtypes = [vp, C.c_int, vp, sz]
    lib.rt_device_variance.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.rt_render_features_chain.argtypes = [vp, vp, C.POINTER(FeatureChainParams)]
    lib.rt_feature_chain_signature.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]


DENOISE_MOMENTS_MIN_COUNT = 4   # RT_DENOISE_MOMENTS_MIN_COUNT: samples from which rt_denoise_moments trusts a pixel's own variance


def moments_prototypes(lib):
    """ctypes prototypes of the sample-moment entry points (RT_OPT_MOMENTS: rt_read_moments & co.)."""
    vp, sz, u32, f32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_float
    f3 = C.POINTER(f32)
    lib.rt_read_moments.argtypes = [vp, vp, sz]
    lib.rt_device_moments.argtypes = [vp, C.POINTER(vp)]
    lib.rt_moments_merge.argtypes = [u32, f3, f32, u32, f3, f32, f3]
    lib.rt_denoise_moments.argtypes = [vp, C.POINTER(DenoiseVarianceParams)]


def prefix_cache_prototypes(lib):
    """ctypes prototype of rt_prefix_cache_stats (RT_OPT_PREFIX_CACHE)."""
    lib.rt_prefix_cache_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.rt_accum_store_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]   # (RT_OPT_ACCUM_STORE)


def lookahead_prototypes(lib):
    """ctypes prototypes of rt_lookahead_stats / rt_lookahead_plan (RT_OPT_LOOKAHEAD)."""
    p64 = C.POINTER(C.c_uint64)
    lib.rt_lookahead_stats.argtypes = [C.c_void_p, p64, p64, p64, p64]
    lib.rt_lookahead_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]


def sample_grid_prototypes(lib):
    """ctypes prototypes of rt_sample_units / rt_sample_grid_stats (RT_OPT_EXACT_GRID)."""
    p64, u32 = C.POINTER(C.c_uint64), C.c_uint32
    lib.rt_sample_units.argtypes = [u32, u32, u32, u32, C.POINTER(u32)]
    lib.rt_sample_grid_stats.argtypes = [C.c_void_p, p64, p64, p64, p64]
    lib.rt_debug_live_list.argtypes = [C.c_void_p, C.POINTER(u32)]
    lib.rt_debug_wave_fixed.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.rt_debug_stage_block.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(u32)]
    lib.rt_debug_queue_pixels.argtypes = [u32, u32, u32, u32, C.POINTER(u32)]
    lib.rt_debug_queue_occupancy.argtypes = [C.c_void_p, u32, C.POINTER(C.c_int)]
    lib.rt_debug_plan_samples.argtypes = [C.POINTER(SampleFacts), C.POINTER(SamplePlan)]
    lib.rt_debug_last_sample_plan.argtypes = [C.c_void_p, C.POINTER(SampleFacts), C.POINTER(SamplePlan)]


class _U32Record(C.Structure):
    """A C struct of uint32_t fields only, made from and turned into a dict."""

    def __init__(self, **kw):
        super().__init__(**{k: int(v) for k, v in kw.items()})

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SampleFacts(_U32Record):
    """rt_sample_facts: what the fused launcher's choice of sample kernel reads"""
    _fields_ = [(k, C.c_uint32) for k in (
        "count", "glog2", "n", "seg_cap", "material_count", "sphere_count", "plane_count", "lens_count", "model_count",
        "sphere_bvh", "mesh_bvh", "walk_jobs", "faces", "cu_count", "count_enabled", "sample_queue", "walk_slices",
        "wave_fill", "moments", "exact", "count_light", "count_heavy")]


PLAN_FIXED, PLAN_QUEUE, PLAN_WALK = 0, 1, 2   # rt_sample_plan.family
PLAN_GENERIC_COUNT = 0xFFFFFFFF               # rt_sample_plan.count_log2 of COUNT_LOG2 = -1


class SamplePlan(_U32Record):
    """rt_sample_plan: the sample kernel's instantiation and launch geometry"""
    _fields_ = [(k, C.c_uint32) for k in (
        "family", "count", "accel", "geom", "waves", "moments", "count_log2", "multi", "pixels_per_wave", "lds_face_f4",
        "lds_bytes", "grid_units", "block_size")]


class CameraFacts(_U32Record):
    """rt_camera_facts: what the choice of kernel of an rt_render_spp_cameras launch reads"""
    _fields_ = [(k, C.c_uint32) for k in (
        "count", "glog2", "n", "material_count", "sphere_count", "plane_count", "lens_count", "model_count", "sphere_bvh",
        "mesh_bvh", "faces", "cu_count", "count_enabled", "sample_queue", "wave_fill", "moments")]


CAMERA_PLAN_FIXED, CAMERA_PLAN_QUEUE = 0, 1   # rt_camera_plan.family
AGAIN_CAMERAS_MAX = 4096                      # RT_AGAIN_CAMERAS_MAX: blocks of an rt_render_again_cameras table


class CameraPlan(_U32Record):
    """rt_camera_plan: the camera launch's kernel and launch geometry"""
    _fields_ = [(k, C.c_uint32) for k in (
        "family", "count", "accel", "geom", "waves", "moments", "pixels_per_wave", "lds_face_f4", "lds_bytes", "grid_units",
        "block_size")]


def camera_prototypes(lib):
    """ctypes prototypes of rt_render_spp_cameras and its plan probes."""
    vp, u32 = C.c_void_p, C.c_uint32
    lib.rt_render_spp_cameras.argtypes = [vp, vp, u32, u32]
    lib.rt_render_again_cameras.argtypes = [vp, vp, u32]
    lib.rt_debug_plan_camera_samples.argtypes = [C.POINTER(CameraFacts), C.POINTER(CameraPlan)]
    lib.rt_debug_last_camera_plan.argtypes = [vp, C.POINTER(CameraFacts), C.POINTER(CameraPlan)]
    lib.rt_render_features_cameras.argtypes = [vp, vp, u32, C.POINTER(FeatureChainParams)]
    lib.rt_read_feature_coverage.argtypes = [vp, vp, C.c_size_t]
    lib.rt_device_feature_coverage.argtypes = [vp, C.POINTER(vp)]
    lib.rt_debug_plan_feature_cameras.argtypes = [C.c_int, C.c_int, u32, C.POINTER(u32)]


# rt_ray (rt_render_rays): origin, random-stream x, direction (used as given), random-stream y — 32 bytes, two float4
RAY = np.dtype([("o", "<f4", (3,)), ("x", "<u4"), ("d", "<f4", (3,)), ("y", "<u4")])
assert RAY.itemsize == 32
MAX_RAYS = 1 << 28          # RT_MAX_RAYS


def check_rays(t):
    """A ray batch as renderRays takes it on the device: a torch tensor of shape (n, 8), float32, contiguous, on a GPU,
    holding rt_ray bits (RAY: the ids are the float words 3 and 7 reinterpreted).  Raises ValueError otherwise, before any
    library call; needs no device.  → n."""
    try:
        import torch
    except ImportError:
        torch = None
    if torch is None or not isinstance(t, torch.Tensor):
        raise ValueError("rays must be a torch tensor on the device (upload a numpy batch with uploadRays)")
    if t.dtype != torch.float32:
        raise ValueError("rays must be float32 (rt_ray bits), not %s" % t.dtype)
    if t.dim() != 2 or t.shape[1] != 8:
        raise ValueError("rays must have shape (n, 8), not %s" % (tuple(t.shape),))
    if t.shape[0] < 1 or t.shape[0] > MAX_RAYS:
        raise ValueError("a ray batch holds 1 .. 2^28 rays, not %d" % t.shape[0])
    if not t.is_contiguous():
        raise ValueError("rays must be contiguous")
    if t.device.type != "cuda":
        raise ValueError("rays must live on the device, not on %s" % t.device)
    return int(t.shape[0])


RAY_SET_MAX = 4096          # RT_RAY_SET_MAX
MAX_RAY_RECORDS = 1 << 31   # n_rays * set_size of one rt_render_ray_sets call


def check_ray_sets(t, set_size):
    """Ray sets as renderRaySets takes them on the device: a torch tensor of shape (n_rays * set_size, 8) or
    (n_rays, set_size, 8), float32, contiguous, on a GPU, holding rt_ray bits ray-major (the set of ray i is records
    i * set_size .. + set_size - 1).  Raises ValueError otherwise, before any library call; needs no device.  → n_rays."""
    try:
        import torch
    except ImportError:
        torch = None
    k = int(set_size)
    if not 1 <= k <= RAY_SET_MAX:
        raise ValueError("a ray set holds 1 .. %d records, not %d" % (RAY_SET_MAX, k))
    if torch is None or not isinstance(t, torch.Tensor):
        raise ValueError("ray sets must be a torch tensor on the device (upload a numpy batch with uploadRays)")
    if t.dtype != torch.float32:
        raise ValueError("ray sets must be float32 (rt_ray bits), not %s" % t.dtype)
    if t.dim() == 3 and t.shape[1] == k and t.shape[2] == 8:
        n = int(t.shape[0])
    elif t.dim() == 2 and t.shape[1] == 8 and t.shape[0] % k == 0:
        n = int(t.shape[0]) // k
    else:
        raise ValueError("ray sets of %d must have shape (n * %d, 8) or (n, %d, 8), not %s" % (k, k, k, tuple(t.shape)))
    if n < 1 or n > MAX_RAYS or n * k > MAX_RAY_RECORDS:
        raise ValueError("ray sets hold 1 .. 2^28 rays and at most 2^31 records, not %d x %d" % (n, k))
    if not t.is_contiguous():
        raise ValueError("ray sets must be contiguous")
    if t.device.type != "cuda":
        raise ValueError("ray sets must live on the device, not on %s" % t.device)
    return n


def check_adaptive_set_size(set_size):
    """The set size of renderAdaptiveRays: 0 (one record per ray) or 1 .. RAY_SET_MAX.  ValueError otherwise.  → int."""
    k = int(set_size)
    if not 0 <= k <= RAY_SET_MAX:
        raise ValueError("set_size is 0 (one record per ray) or 1 .. %d, not %d" % (RAY_SET_MAX, k))
    return k


def check_adaptive_rays(t, set_size, width, height):
    """A device batch as renderAdaptiveRays takes it: check_rays' tensor (set_size 0) or check_ray_sets' (set_size 1 ..
    RAY_SET_MAX) holding exactly one ray per pixel of the width x height frame.  Raises ValueError otherwise, before any
    library call; needs no device.  → n_rays."""
    k = check_adaptive_set_size(set_size)
    n = check_ray_sets(t, k) if k else check_rays(t)
    if n != int(width) * int(height):
        raise ValueError("an adaptive frame takes one ray per pixel: %d rays for %d x %d" % (n, width, height))
    return n


def check_ray_target(t, n):
    """The external target of renderRays: a torch (n, 4) float32 contiguous device tensor.  ValueError otherwise."""
    try:
        import torch
    except ImportError:
        torch = None
    if torch is None or not isinstance(t, torch.Tensor):
        raise ValueError("out must be a torch tensor on the device")
    if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (n, 4):
        raise ValueError("out must be float32 of shape (%d, 4), not %s %s" % (n, t.dtype, tuple(t.shape)))
    if not t.is_contiguous() or t.device.type != "cuda":
        raise ValueError("out must be a contiguous device tensor")


def check_ray_bounds(t, records):
    """The per-record bounds of occludedRays: a torch float32 contiguous device tensor of `records` elements — (records,),
    or (n_rays, set_size) with n_rays * set_size == records.  ValueError otherwise, before any library call."""
    try:
        import torch
    except ImportError:
        torch = None
    if torch is None or not isinstance(t, torch.Tensor):
        raise ValueError("bounds must be a torch tensor on the device")
    if t.dtype != torch.float32:
        raise ValueError("bounds must be float32, not %s" % t.dtype)
    if t.dim() not in (1, 2) or t.numel() != int(records):
        raise ValueError("bounds must hold one float per record (%d), not shape %s" % (records, tuple(t.shape)))
    if not t.is_contiguous() or t.device.type != "cuda":
        raise ValueError("bounds must be a contiguous device tensor")


FEATURE_FLOATS = 20   # an rt_feature record as float32 words (FEATURE.itemsize / 4)


def check_feature_target(t, n):
    """The output of intersectRays: a torch (n, 20) float32 contiguous device tensor (n rt_feature records).  ValueError
    otherwise."""
    try:
        import torch
    except ImportError:
        torch = None
    if torch is None or not isinstance(t, torch.Tensor):
        raise ValueError("out must be a torch tensor on the device")
    if t.dtype != torch.float32 or tuple(t.shape) != (int(n), FEATURE_FLOATS):
        raise ValueError("out must be float32 of shape (%d, %d), not %s %s" % (n, FEATURE_FLOATS, t.dtype, tuple(t.shape)))
    if not t.is_contiguous() or t.device.type != "cuda":
        raise ValueError("out must be a contiguous device tensor")


def check_count_target(t, n):
    """The output of occludedRays: a torch (n,) int32 contiguous device tensor.  ValueError otherwise."""
    try:
        import torch
    except ImportError:
        torch = None
    if torch is None or not isinstance(t, torch.Tensor):
        raise ValueError("out must be a torch tensor on the device")
    if t.dtype != torch.int32 or tuple(t.shape) != (int(n),):
        raise ValueError("out must be int32 of shape (%d,), not %s %s" % (n, t.dtype, tuple(t.shape)))
    if not t.is_contiguous() or t.device.type != "cuda":
        raise ValueError("out must be a contiguous device tensor")


HEMI_FACE_FORWARD = 1       # RT_HEMI_FACE_FORWARD: use -normal where dot(normal, record.dir) > 0


class HemisphereParams(C.Structure):
    """rt_hemisphere_params (include/rt_amd.h)."""
    _fields_ = [("k", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint64), ("offset", C.c_float), ("t_max", C.c_float)]


def check_hemispheres(features, n, k, flags, offset, counts, rays_out, width, height, world=1):
    """What rt_occluded_hemispheres refuses with RT_EINVAL, restated without a device: `features` an (n, 20) float32
    contiguous device tensor of rt_feature records or None (the context's own width x height records: n must be their
    number), 1 <= n <= MAX_RAYS, 1 <= k <= RAY_SET_MAX, n * k <= 2^31, flags within HEMI_FACE_FORWARD, a finite offset,
    `counts` an (n,) int32 and `rays_out` an (n * k, 8) or (n, k, 8) float32 contiguous device tensor — each may be None,
    not both — 16-byte aligned records, an unsharded context.  ValueError otherwise; → HemisphereParams' k and flags."""
    n, k, flags = check_hemisphere_source(features, n, k, flags, offset, width, height, world)
    if counts is None and rays_out is None:
        raise ValueError("a hemisphere query needs counts, rays_out or both")
    if counts is not None:
        check_count_target(counts, n)
    if rays_out is not None:
        if check_ray_sets(rays_out, k) != n:
            raise ValueError("rays_out must hold %d x %d records, not shape %s" % (n, k, tuple(rays_out.shape)))
        if rays_out.data_ptr() % 16:
            raise ValueError("rays_out must be 16-byte aligned")
    return k, flags


def check_hemisphere_source(features, n, k, flags, offset, width, height, world=1):
    """The rules rt_occluded_hemispheres and rt_render_hemispheres share, for the records and the parameters (see
    check_hemispheres).  ValueError otherwise; → (n, k, flags) as ints."""
    n, k, flags = int(n), int(k), int(flags)
    if int(world) > 1:
        raise ValueError("hemisphere queries on a sharded context: shard the records instead")
    if not 1 <= n <= MAX_RAYS:
        raise ValueError("a hemisphere query takes 1 .. %d records, not %d" % (MAX_RAYS, n))
    if not 1 <= k <= RAY_SET_MAX:
        raise ValueError("a hemisphere holds 1 .. %d rays, not %d" % (RAY_SET_MAX, k))
    if n * k > MAX_RAY_RECORDS:
        raise ValueError("%d records x %d rays exceed 2^31 rays" % (n, k))
    if flags & ~HEMI_FACE_FORWARD:
        raise ValueError("unknown hemisphere flags 0x%x" % flags)
    if not np.isfinite(offset) or abs(float(offset)) > float(np.finfo(np.float32).max):   # (finite as a float)
        raise ValueError("the hemisphere offset must be finite, not %r" % (offset,))
    if features is None:
        if n != int(width) * int(height):
            raise ValueError("the context's feature records are %d x %d, not %d" % (width, height, n))
    else:
        check_feature_target(features, n)
        if features.data_ptr() % 16:
            raise ValueError("features must be 16-byte aligned")
    return n, k, flags


def check_hemisphere_target(t, n):
    """The external target of renderHemispheres: renderRays' (check_ray_target) — a torch (n, 4) float32 contiguous device
    tensor — 16-byte aligned.  ValueError otherwise."""
    check_ray_target(t, int(n))
    if t.data_ptr() % 16:
        raise ValueError("out must be 16-byte aligned")


def check_gather(features, n, k, flags, offset, first_sample, n_samples, out, width, height, world=1):
    """What rt_render_hemispheres refuses with RT_EINVAL, restated without a device: check_hemisphere_source's rules for the
    records and the parameters, then n_samples (None: k) at least 1 with first_sample + n_samples - 1 <= MAX_SAMPLE, and
    `out` a check_hemisphere_target or None (the accumulator: n must be width x height).  ValueError otherwise; → (k, flags,
    first_sample, n_samples) as ints."""
    n, k, flags = check_hemisphere_source(features, n, k, flags, offset, width, height, world)
    first_sample, n_samples = int(first_sample), k if n_samples is None else int(n_samples)
    if n_samples < 1 or first_sample < 0 or first_sample + n_samples - 1 > MAX_SAMPLE:
        raise ValueError("samples %d..+%d: 1 or more, up to the limit %d" % (first_sample, n_samples, MAX_SAMPLE))
    if out is None:
        if n != int(width) * int(height):
            raise ValueError("%d records into the accumulator of a %d x %d frame" % (n, width, height))
    else:
        check_hemisphere_target(out, n)
    return k, flags, first_sample, n_samples


def feature_records(t):
    """intersectRays' (n, 20) float32 tensor → (n,) FEATURE records on the host (a copy; the caller has synchronised)."""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(FEATURE).reshape(-1)


def ray_prototypes(lib):
    """ctypes prototypes of the caller-supplied-ray entry points (rt_render_rays & co.)."""
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.rt_upload_rays.argtypes = [vp, vp, sz]
    lib.rt_device_rays.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    lib.rt_render_rays.argtypes = [vp, vp, sz, u32, u32, vp]
    lib.rt_render_ray_sets.argtypes = [vp, vp, sz, u32, u32, u32, vp]
    lib.rt_render_features_rays.argtypes = [vp, vp, sz, C.POINTER(FeatureChainParams)]
    lib.rt_debug_last_ray_plan.argtypes = [vp, C.POINTER(CameraFacts), C.POINTER(CameraPlan)]
    lib.rt_render_adaptive_rays.argtypes = [vp, vp, sz, u32, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStats)]
    lib.rt_render_adaptive_variance_rays.argtypes = [vp, vp, sz, u32, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStats)]
    lib.rt_intersect_rays.argtypes = [vp, vp, sz, C.POINTER(FeatureChainParams), vp]
    lib.rt_occluded_rays.argtypes = [vp, vp, sz, u32, vp, C.c_float, vp]
    lib.rt_occluded_hemispheres.argtypes = [vp, vp, sz, C.POINTER(HemisphereParams), vp, vp]
    lib.rt_render_hemispheres.argtypes = [vp, vp, sz, C.POINTER(HemisphereParams), u32, u32, vp]
    lib.rt_device_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.rt_device_free.argtypes = [vp, vp]
    lib.rt_device_copy.argtypes = [vp, vp, vp, sz, C.c_int]


# the caps of the sample kernels' LDS tables (csrc/pt_types.hpp PT_LDS_MATERIALS, PT_LDS_WINNERS, PT_LDS_PLANES)
LDS_MATERIALS, LDS_WINNERS, LDS_PLANES = 64, 64, 16


def stage_block_layout(n_materials, n_spheres, n_planes):
    """(first row of the materials, of the sphere records, of the plane records, rows in all) of the staged scene block
    (rt_debug_stage_block): two rows per material, two per sphere, one per plane; a set over its cap has no rows."""
    nm = 2 * n_materials if n_materials <= LDS_MATERIALS else 0
    nw = 2 * n_spheres if n_spheres <= LDS_WINNERS else 0
    npl = n_planes if n_planes <= LDS_PLANES else 0
    return 0, nm, nm + nw, nm + nw + npl


def queue_sums_prototypes(lib):
    """ctypes prototype of rt_debug_queue_sums (the sample queue's per-pixel summation, one wave)."""
    u32 = C.c_uint32
    lib.rt_debug_queue_sums.argtypes = [C.c_void_p, C.c_void_p, u32, u32, u32, C.c_void_p]


def split_features(rec):
    """(H, W) FEATURE records → dict of (H, W, ...) arrays (RayTracer.features())."""
    return {"position": rec["pos"].copy(), "depth": rec["t"].copy(), "normal": rec["normal"].copy(),
            "albedo": rec["albedo"].copy(), "object": rec["object"].copy(), "material": rec["material"].copy(),
            "face": rec["face"].copy(), "direction": rec["dir"].copy(),
            "uv": np.stack([rec["u"], rec["v"]], axis=-1), "texture": rec["tex"].copy(),
            "hit": (rec["flags"] & FEATURE_HIT) != 0,
            # rt_render_features_chain (all 0 / False in first-hit records): followed vertices, the signature's upper half
            # (as flags & 0xFFFF0000), the cut flag, and flags >> 8 — the word RT_DENOISE_SPLIT_CHAINS compares
            "chain_length": ((rec["flags"] >> 8) & 31).astype(np.uint32),
            "chain_signature": (rec["flags"] & np.uint32(0xFFFF0000)).astype(np.uint32),
            "cut": (rec["flags"] & FEATURE_CUT) != 0, "chain_word": (rec["flags"] >> 8).astype(np.uint32),
            # rt_render_features_cameras (False otherwise): the pixel's samples fall into more than one group
            "mixed": (rec["flags"] & FEATURE_MIXED) != 0}


def ptr(a):
    """void* of a numpy array (None/empty → NULL)."""
    if a is None or a.size == 0:
        return None
    return a.ctypes.data_as(C.c_void_p)
