"""RayTracer — host-side mirror of the reference's class (include/raytracer.h:17-47,
src/raytracer.cpp:24-174) over the C ABI of librt_amd.so (include/rt_amd.h).

Same surface as the reference: ``RayTracer(w, h, kernel_path)``, ``render(camera)``,
``renderAgain(camera)``, ``transferImage()``, plus the two methods the reference
declares but never defines (``resize``, ``setTime``) and the native fused path
(``renderSamples``).  The HIP library is the only compute path: if it cannot be
loaded, or no gfx950 device is present, construction raises — there is no CPU
fallback here.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from .scene import SceneCreator

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librt_amd.so")

# every symbol include/rt_amd.h declares
SYMBOLS = (
    "rt_abi_version", "rt_last_error", "rt_create", "rt_destroy", "rt_resize", "rt_set_stream", "rt_set_scene",
    "rt_set_textures", "rt_set_seed", "rt_set_random_table", "rt_get_random_table", "rt_make_random_table",
    "rt_set_shard", "rt_render", "rt_render_again", "rt_sample_counter", "rt_clear", "rt_render_spp", "rt_resolve",
    "rt_sync", "rt_trace_samples", "rt_read_image", "rt_read_linear", "rt_device_image", "rt_device_accum",
    "rt_enable_counters", "rt_reset_counters", "rt_get_counters", "rt_counters_bytes", "rt_last_kernel_ms",
    "rt_kernel_ms_history", "rt_stage_ms_history", "rt_debug_hit", "rt_debug_material", "rt_debug_div3", "rt_device_info", "rt_set_option", "rt_shard_slots", "rt_pack_accum", "rt_unpack_accum",
    "rt_get_debug_counters", "rt_debug_check_accel", "rt_walk_overflow", "rt_debug_builtin",
    "rt_render_adaptive", "rt_read_sample_counts", "rt_read_block_error",
    "rt_render_features", "rt_read_features", "rt_device_features", "rt_render_features_chain", "rt_feature_chain_signature",
    "rt_denoise", "rt_read_denoised", "rt_device_denoised",
    "rt_denoise_variance", "rt_read_variance", "rt_device_variance",
    "rt_read_moments", "rt_device_moments", "rt_moments_merge", "rt_denoise_moments",
    "rt_prefix_cache_stats", "rt_accum_store_stats", "rt_lookahead_stats", "rt_lookahead_plan",
    "rt_sample_units", "rt_sample_grid_stats", "rt_debug_live_list", "rt_debug_wave_fixed", "rt_debug_stage_block", "rt_debug_queue_pixels", "rt_debug_queue_occupancy", "rt_debug_queue_sums",
    "rt_debug_plan_samples", "rt_debug_last_sample_plan",
    "rt_render_spp_cameras", "rt_debug_plan_camera_samples", "rt_debug_last_camera_plan",
    "rt_render_features_cameras", "rt_read_feature_coverage", "rt_device_feature_coverage", "rt_debug_plan_feature_cameras",
    "rt_render_adaptive_cameras", "rt_render_again_cameras",
    "rt_render_adaptive_variance", "rt_render_adaptive_variance_cameras", "rt_read_pixel_error", "rt_device_pixel_error",
    "rt_upload_rays", "rt_device_rays", "rt_render_rays", "rt_render_features_rays", "rt_debug_last_ray_plan",
    "rt_render_ray_sets",
    "rt_render_adaptive_rays", "rt_render_adaptive_variance_rays",
    "rt_intersect_rays", "rt_occluded_rays", "rt_device_alloc", "rt_device_free", "rt_device_copy",
    "rt_occluded_hemispheres", "rt_render_hemispheres",
)

# rt_set_option: options and the arithmetic policies of RT_OPT_ARITH (include/rt_amd.h)
OPT_PREFIX_SHARING, OPT_MAX_THREADS_PER_LAUNCH, OPT_SAMPLE_QUEUE, OPT_ACCEL, OPT_WALK_SLICES, OPT_ARITH, OPT_PREFIX_TREE, OPT_WAVE_FILL = 1, 2, 3, 4, 5, 6, 7, 8
OPT_PREFIX_CACHE = 9
OPT_LOOKAHEAD = 10
OPT_EXACT_GRID = 11
OPT_MOMENTS = 12
OPT_ACCUM_STORE = 13
ARITH_IEEE, ARITH_ROCM_OCL_NOCONTRACT, ARITH_ROCM_OCL = 0, 1, 2
# rt_render_features_chain: the material types a chain is followed through
FOLLOW_REFLECTIVE, FOLLOW_REFRACTIVE, FOLLOW_DIELECTRIC = _abi.FOLLOW_REFLECTIVE, _abi.FOLLOW_REFRACTIVE, _abi.FOLLOW_DIELECTRIC
FOLLOW_ALL = FOLLOW_REFLECTIVE | FOLLOW_REFRACTIVE | FOLLOW_DIELECTRIC
ARITH_NAMES = {"ieee": ARITH_IEEE, "rocm-opencl-nocontract": ARITH_ROCM_OCL_NOCONTRACT, "rocm-opencl": ARITH_ROCM_OCL}


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("librt_amd: %s (code %d)" % (msg, code))
        self.code = code


_lib = None


def load_library(path=LIB_PATH):
    """dlopen librt_amd.so and type its entry points.  Raises if it is missing:
    build it with ``python -c 'import __graft_entry__ as g; g.build()'``."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(path):
        raise OSError("%s not found — the HIP library is not built (run __graft_entry__.build()); "
                      "there is no CPU fallback" % path)
    # PyTorch's ROCm wheel bundles its own libamdhip64.so.7.  A process must hold ONE HIP runtime:
    # if librt_amd.so pulled in /opt/rocm's copy first, a later `import torch` would find "No HIP
    # GPUs".  Importing torch first (when it is installed) makes both bind to the same runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for s in SYMBOLS:
        getattr(lib, s)  # AttributeError if the library does not export what the header declares
    vp, u32, u64, sz, fp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.POINTER(C.c_float)
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_last_error.argtypes = [vp]
    lib.rt_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.rt_destroy.argtypes = [vp]
    lib.rt_destroy.restype = None
    lib.rt_resize.argtypes = [vp, C.c_int, C.c_int]
    lib.rt_set_stream.argtypes = [vp, vp]
    lib.rt_set_scene.argtypes = [vp, C.POINTER(_abi.SceneDesc)]
    lib.rt_set_textures.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    lib.rt_set_seed.argtypes = [vp, u64]
    lib.rt_set_random_table.argtypes = [vp, vp, sz]
    lib.rt_get_random_table.argtypes = [vp, vp, sz]
    lib.rt_make_random_table.argtypes = [u64, vp, sz]
    lib.rt_set_shard.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.rt_render.argtypes = [vp, vp]
    lib.rt_render_again.argtypes = [vp, vp]
    lib.rt_sample_counter.argtypes = [vp, C.POINTER(u32)]
    lib.rt_clear.argtypes = [vp]
    lib.rt_render_spp.argtypes = [vp, vp, u32, u32]
    lib.rt_resolve.argtypes = [vp]
    lib.rt_sync.argtypes = [vp]
    lib.rt_trace_samples.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    lib.rt_read_image.argtypes = [vp, vp, sz]
    lib.rt_read_linear.argtypes = [vp, vp, sz]
    lib.rt_device_image.argtypes = [vp, C.POINTER(vp)]
    lib.rt_device_accum.argtypes = [vp, C.POINTER(vp)]
    lib.rt_enable_counters.argtypes = [vp, C.c_int]
    lib.rt_reset_counters.argtypes = [vp]
    lib.rt_get_counters.argtypes = [vp, C.POINTER(_abi.Counters)]
    lib.rt_counters_bytes.argtypes = [C.POINTER(_abi.Counters)]
    lib.rt_counters_bytes.restype = u64
    lib.rt_last_kernel_ms.argtypes = [vp, fp]
    lib.rt_kernel_ms_history.argtypes = [vp, fp, sz, C.POINTER(sz)]
    lib.rt_stage_ms_history.argtypes = [vp, fp, fp, sz, C.POINTER(sz)]
    lib.rt_debug_hit.argtypes = [vp, C.c_int, vp, vp, vp, sz, vp]
    lib.rt_debug_material.argtypes = [vp, C.c_int, vp, sz, vp]
    lib.rt_debug_div3.argtypes = [vp, vp, sz, vp]
    lib.rt_set_option.argtypes = [vp, C.c_int, C.c_int]
    lib.rt_shard_slots.argtypes = [vp, C.c_int, C.POINTER(u32)]
    lib.rt_pack_accum.argtypes = [vp, vp, sz]
    lib.rt_unpack_accum.argtypes = [vp, vp, sz, C.c_int, C.c_int]
    lib.rt_device_info.argtypes = [vp, C.c_char_p, sz, C.POINTER(C.c_int), C.c_char_p, sz]
    lib.rt_walk_overflow.argtypes = [vp, C.POINTER(u32)]
    lib.rt_debug_builtin.argtypes = [vp, C.c_int, vp, sz, vp]
    _abi.adaptive_prototypes(lib)
    _abi.denoise_prototypes(lib)
    _abi.moments_prototypes(lib)
    _abi.prefix_cache_prototypes(lib)
    _abi.lookahead_prototypes(lib)
    _abi.sample_grid_prototypes(lib)
    _abi.queue_sums_prototypes(lib)
    _abi.camera_prototypes(lib)
    _abi.ray_prototypes(lib)
    if lib.rt_abi_version() != _abi.RT_ABI_VERSION:
        raise OSError("librt_amd.so ABI %d != expected %d" % (lib.rt_abi_version(), _abi.RT_ABI_VERSION))
    _lib = lib
    return lib


def check_accel(scene):
    """Host-only self-check of what rt_set_scene would upload for `scene` (no device needed): the scene is validated
    and prepared as rt_set_scene does it, and the invariants of the prepared structures are verified.
    → stats dict ("digest": FNV-1a-64 of the prepared arrays); raises RtError with the validation error or the
    violated invariant."""
    lib = load_library()
    d = scene.desc()
    stats = (C.c_uint64 * 8)()
    err = C.create_string_buffer(256)
    rc = lib.rt_debug_check_accel(C.byref(d), stats, err, 256)
    if rc:
        raise RtError(rc, err.value.decode() or "accel check failed")
    keys = ("sphere_nodes", "sphere_leaves", "sphere_depth", "mesh_nodes", "mesh_leaves", "mesh_depth", "meshes", "digest")
    return dict(zip(keys, [int(v) for v in stats]))


def make_random_table(seed):
    """The table rt_set_seed(seed) uploads (host-only; no device needed)."""
    lib = load_library()
    out = np.empty(_abi.RANDOM_TABLE_FLOATS, dtype=np.float32)
    rc = lib.rt_make_random_table(seed, out.ctypes.data, out.size)
    if rc:
        raise RtError(rc, lib.rt_last_error(None).decode())
    return out


def lookahead_plan(width, height, option=16, sample_counter=0):
    """Samples the look-ahead launch of a renderAgain call would trace (rt_lookahead_plan; host-only, no device needed):
    0 = that call runs the direct kernel."""
    lib = load_library()
    out = C.c_uint32()
    rc = lib.rt_lookahead_plan(int(width), int(height), int(option), int(sample_counter), C.byref(out))
    if rc:
        raise RtError(rc, lib.rt_last_error(None).decode())
    return int(out.value)


def sample_units(seg_cap, pixels_per_unit, count_light, count_heavy):
    """Workgroups of a sample-kernel launch that own a pixel, for a live list of capacity `seg_cap` whose two counters
    read `count_light` and `count_heavy` (rt_sample_units; host-only, no device needed): what a launch under
    OPT_EXACT_GRID has."""
    lib = load_library()
    out = C.c_uint32()
    rc = lib.rt_sample_units(int(seg_cap), int(pixels_per_unit), int(count_light), int(count_heavy), C.byref(out))
    if rc:
        raise RtError(rc, lib.rt_last_error(None).decode())
    return int(out.value)


def moments_merge(nA, sumA, m2A, nB, sumB, m2B):
    """M2 of the union of two partial states (count, RGB sum, centred second luminance moment) of a pixel
    (rt_moments_merge; host-only, no device needed): the float32 function the kernels call."""
    lib = load_library()
    a = (C.c_float * 3)(*[float(v) for v in sumA])
    b = (C.c_float * 3)(*[float(v) for v in sumB])
    out = C.c_float()
    rc = lib.rt_moments_merge(int(nA), a, float(m2A), int(nB), b, float(m2B), C.byref(out))
    if rc:
        raise RtError(rc, lib.rt_last_error(None).decode())
    return np.float32(out.value)


def feature_chain_signature(objects):
    """Signature of a chain through the listed object ids, in path order (rt_feature_chain_signature; host-only, no device
    needed): the function the kernel calls.  A record's flags hold its upper 16 bits."""
    lib = load_library()
    o = np.ascontiguousarray(objects, dtype=np.uint32).reshape(-1)
    out = C.c_uint32()
    rc = lib.rt_feature_chain_signature(o.ctypes.data if len(o) else None, len(o), C.byref(out))
    if rc:
        raise RtError(rc, lib.rt_last_error(None).decode())
    return int(out.value)


def _cam_block(camera):
    block = camera.transferData() if hasattr(camera, "transferData") else camera
    block = np.ascontiguousarray(block, dtype=np.float32)
    if block.shape != (12,):
        raise ValueError("camera block must be 12 floats")
    return block


class DeviceBuffer:
    """A W×H×4 float32 device buffer owned by a RayTracer, exposed through
    ``__cuda_array_interface__`` so torch can wrap it without a copy
    (``torch.as_tensor(buf, device="cuda")``) for the RCCL reduce."""

    def __init__(self, ptr, h, w, owner):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": (h, w, 4), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 3, "strides": None}


def queue_pixels(count, waves_per_simd=6, static_float4=0, granule=0):
    """Pixels a wave of the sample queue owns (rt_debug_queue_pixels: the launcher's own function; granule 0 = the shipped one)."""
    n = C.c_uint32()
    rc = load_library().rt_debug_queue_pixels(int(count), int(waves_per_simd), int(static_float4), int(granule), C.byref(n))
    if rc:
        raise RtError(rc, "rt_debug_queue_pixels: invalid argument")
    return int(n.value)


def plan_samples(**facts):
    """The sample-kernel launch the fused launcher plans for these facts (rt_debug_plan_samples: the launcher's own function;
    host-only, no device needed): the fields of _abi.SampleFacts (those left out are 0) → the fields of _abi.SamplePlan."""
    f, p = _abi.SampleFacts(**facts), _abi.SamplePlan()
    rc = load_library().rt_debug_plan_samples(C.byref(f), C.byref(p))
    if rc:
        raise RtError(rc, "rt_debug_plan_samples: invalid argument")
    return p.as_dict()


def plan_camera_samples(**facts):
    """The launch rt_render_spp_cameras' launcher plans for these facts (rt_debug_plan_camera_samples: the launcher's own
    function; host-only, no device needed): the fields of _abi.CameraFacts (those left out are 0) → those of _abi.CameraPlan."""
    f, p = _abi.CameraFacts(**facts), _abi.CameraPlan()
    rc = load_library().rt_debug_plan_camera_samples(C.byref(f), C.byref(p))
    if rc:
        raise RtError(rc, "rt_debug_plan_camera_samples: invalid argument")
    return p.as_dict()


def plan_feature_cameras(width, height, n):
    """The launch rt_render_features_cameras plans for a width x height frame and n camera blocks
    (rt_debug_plan_feature_cameras: the launcher's own function; host-only, no device needed) → (log2 of the lanes per
    pixel, workgroups, threads per workgroup)."""
    out = (C.c_uint32 * 3)()
    rc = load_library().rt_debug_plan_feature_cameras(int(width), int(height), int(n), out)
    if rc:
        raise RtError(rc, "rt_debug_plan_feature_cameras: invalid argument")
    return tuple(int(v) for v in out)


def _cam_blocks(blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.float32)
    if blocks.ndim != 2 or blocks.shape[1] != 12:
        raise ValueError("camera blocks must be n x 12 floats")
    return blocks


class RayTracer:
    # the reference hard-codes "assets/scenes/scene.scene" relative to the working directory (src/raytracer.cpp:95): that
    # path is tried as written first, then this repository's own file of that name
    DEFAULT_SCENE = os.path.join("assets", "scenes", "scene.scene")
    REPO_DEFAULT_SCENE = os.path.join(os.path.dirname(_HERE), "assets", "scenes", "scene.scene")

    def __init__(self, w, h, kernel_path=None, scene=None, device=0, seed=0xC0FFEE):
        """``kernel_path`` is accepted for source compatibility with
        RayTracer(w, h, "kernels/raytracer.cl") and ignored: the kernels are
        compiled into librt_amd.so.  ``scene``: a SceneCreator, a .scene path, or
        None for the default scene file (the reference hard-codes
        "assets/scenes/scene.scene", src/raytracer.cpp:95)."""
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.rt_create(device, w, h, C.byref(self._ctx))
        if rc:
            self._ctx = C.c_void_p()
            raise RtError(rc, self._lib.rt_last_error(None).decode())
        self.width, self.height = w, h
        self._device = int(device)   # (where intersectRays / occludedRays make their outputs)
        if seed != 0xC0FFEE:
            self.setSeed(seed)
        if scene is None:
            scene = self.DEFAULT_SCENE if os.path.isfile(self.DEFAULT_SCENE) else self.REPO_DEFAULT_SCENE
        if isinstance(scene, str):
            path = scene
            scene = SceneCreator()
            scene.loadScene(path)
            scene.loadTextures()
        self.setScene(scene)

    # -- plumbing -------------------------------------------------------------------
    def _check(self, rc):
        if rc:
            raise RtError(rc, self._lib.rt_last_error(self._ctx).decode())

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.rt_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs ---------------------------------------------------------------------
    def setScene(self, scene):
        self.scene = scene
        d = scene.desc()
        self._check(self._lib.rt_set_scene(self._ctx, C.byref(d)))
        tex, tw, th, layers = scene.texture_args()
        self._check(self._lib.rt_set_textures(self._ctx, tex, tw, th, layers))

    def setSeed(self, seed):
        self._check(self._lib.rt_set_seed(self._ctx, seed))

    def setRandomTable(self, table):
        table = np.ascontiguousarray(table, dtype=np.float32)
        self._check(self._lib.rt_set_random_table(self._ctx, table.ctypes.data, table.size))

    def getRandomTable(self):
        out = np.empty(_abi.RANDOM_TABLE_FLOATS, dtype=np.float32)
        self._check(self._lib.rt_get_random_table(self._ctx, out.ctypes.data, out.size))
        return out

    def setShard(self, rank, world, tile_w=8, tile_h=8):
        self._check(self._lib.rt_set_shard(self._ctx, rank, world, tile_w, tile_h))
        self._world = int(world)   # (check_hemispheres restates the library's refusal of sharded contexts)

    OPT_PREFIX_SHARING, OPT_MAX_THREADS_PER_LAUNCH, OPT_SAMPLE_QUEUE, OPT_ACCEL, OPT_WALK_SLICES, OPT_ARITH, OPT_PREFIX_TREE, OPT_WAVE_FILL = 1, 2, 3, 4, 5, 6, 7, 8
    OPT_PREFIX_CACHE = 9
    OPT_LOOKAHEAD = 10
    OPT_EXACT_GRID = 11
    OPT_MOMENTS = 12
    OPT_ACCUM_STORE = 13

    def setOption(self, option, value):
        self._check(self._lib.rt_set_option(self._ctx, option, int(value)))

    def shardSlots(self, world):
        n = C.c_uint32()
        self._check(self._lib.rt_shard_slots(self._ctx, world, C.byref(n)))
        return n.value

    def packAccum(self, device_ptr, nbytes):
        """This rank's owned accumulator pixels → device buffer (slot order)."""
        self._check(self._lib.rt_pack_accum(self._ctx, C.c_void_p(device_ptr), nbytes))

    def unpackAccum(self, device_ptr, nbytes, src_rank, world):
        self._check(self._lib.rt_unpack_accum(self._ctx, C.c_void_p(device_ptr), nbytes, src_rank, world))

    def setStream(self, hip_stream):
        self._check(self._lib.rt_set_stream(self._ctx, C.c_void_p(hip_stream or 0)))

    def resize(self, w, h):
        self._check(self._lib.rt_resize(self._ctx, w, h))
        self.width, self.height = w, h

    def setTime(self, time):
        """Declared, never defined in the reference (include/raytracer.h:45); a stub."""

    # -- rendering --------------------------------------------------------------------
    def render(self, camera):
        self._check(self._lib.rt_render(self._ctx, _cam_block(camera).ctypes.data))

    def renderAgain(self, camera):
        self._check(self._lib.rt_render_again(self._ctx, _cam_block(camera).ctypes.data))

    def renderAgainCameras(self, blocks):
        """renderAgain through a cyclic schedule of camera blocks (n x 12 floats, e.g. Camera.sampleBlocks: progressive
        anti-aliasing, depth of field; rt_render_again_cameras): the call that makes sample s looks through
        blocks[s % n].  Same bits as renderAgain(blocks[s % n]); while the calls repeat one table, RT_OPT_LOOKAHEAD
        serves them from one camera launch per batch."""
        blocks = _cam_blocks(blocks)
        self._check(self._lib.rt_render_again_cameras(self._ctx, blocks.ctypes.data if len(blocks) else None, len(blocks)))

    @property
    def sample_counter(self):
        v = C.c_uint32()
        self._check(self._lib.rt_sample_counter(self._ctx, C.byref(v)))
        return v.value

    def clear(self):
        self._check(self._lib.rt_clear(self._ctx))

    def renderSamples(self, camera, first_sample, n_samples):
        """Fused path: samples first..first+n-1 of every owned pixel in one launch (async)."""
        self._check(self._lib.rt_render_spp(self._ctx, _cam_block(camera).ctypes.data, first_sample, n_samples))

    def renderSamplesCameras(self, blocks, first_sample=0):
        """Samples first..first+n-1 of every owned pixel, sample first + j through camera block blocks[j] (n x 12 floats,
        e.g. Camera.sampleBlocks: pixel jitter, depth of field; rt_render_spp_cameras, async).  Adds to the accumulator
        like renderSamples; n identical blocks give renderSamples' bits."""
        blocks = _cam_blocks(blocks)
        self._check(self._lib.rt_render_spp_cameras(self._ctx, blocks.ctypes.data if len(blocks) else None, first_sample, len(blocks)))

    def renderFrameCameras(self, blocks):
        """clear + renderSamplesCameras(blocks, 0) + resolve + sync → gamma image (h,w,4)."""
        self.clear()
        self.renderSamplesCameras(blocks, 0)
        self.resolve()
        return self.transferImage()

    def lastCameraPlan(self):
        """(facts, plan) dicts of the last renderSamplesCameras launch (rt_debug_last_camera_plan)."""
        f, p = _abi.CameraFacts(), _abi.CameraPlan()
        self._check(self._lib.rt_debug_last_camera_plan(self._ctx, C.byref(f), C.byref(p)))
        return f.as_dict(), p.as_dict()

    # -- caller-supplied rays ---------------------------------------------------------------
    def uploadRays(self, rays):
        """Copies a host batch of rays — an _abi.RAY array (rays.pack_rays and the generators of rays.py make them), or
        (n, 8) float32 holding the same bits — into the context's own ray buffer (rt_upload_rays); renderRays(None, ...)
        and renderFeaturesRays(None) then trace them.  → n."""
        rays = np.asarray(rays)
        if rays.dtype == _abi.RAY:
            rays = np.ascontiguousarray(rays).reshape(-1)
        elif rays.dtype == np.float32 and rays.ndim == 2 and rays.shape[1] == 8:
            rays = np.ascontiguousarray(rays)
        else:
            raise ValueError("rays must be an _abi.RAY array or (n, 8) float32")
        n = len(rays)
        self._check(self._lib.rt_upload_rays(self._ctx, rays.ctypes.data if n else None, n))
        return n

    def deviceRays(self):
        """(device address, count) of the uploaded rays (rt_device_rays)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.rt_device_rays(self._ctx, C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def _ray_args(self, rays):
        """→ (device pointer or None, n, what must stay alive until the call has been enqueued)"""
        if rays is None:
            return None, self.deviceRays()[1], None
        if isinstance(rays, np.ndarray):
            return None, self.uploadRays(rays), None
        n = _abi.check_rays(rays)
        return C.c_void_p(rays.data_ptr()), n, rays

    def renderRays(self, rays, first_sample, n_samples, out=None):
        """Samples first..first+n-1 of every ray of the batch (rt_render_rays, asynchronous on the context's stream).
        `rays`: a torch device tensor (n, 8) float32 holding rt_ray bits, read in place; None: the uploaded rays; a
        numpy batch is uploaded first.  `out`: a torch device tensor (n, 4) float32 the sums and counts are ADDED to, in
        place; None: the accumulator (n == w * h, ray i = pixel i), after which resolve, the denoisers and the moments
        work as for a camera frame.  Work queued on another stream that writes `rays` / `out` is the caller's to order."""
        ptr, n, _keep = self._ray_args(rays)
        target = None
        if out is not None:
            _abi.check_ray_target(out, n)
            target = C.c_void_p(out.data_ptr())
        self._check(self._lib.rt_render_rays(self._ctx, ptr, n, int(first_sample), int(n_samples), target))

    def _ray_set_args(self, rays, set_size):
        """→ (device pointer or None, n_rays, set_size, what must stay alive until the call has been enqueued) of a call
        that takes ray sets: a device tensor as check_ray_sets has it, None for the uploaded records, or a numpy batch,
        which is uploaded first."""
        k = int(set_size)
        if not 1 <= k <= _abi.RAY_SET_MAX:
            raise ValueError("a ray set holds 1 .. %d records, not %d" % (_abi.RAY_SET_MAX, k))
        if rays is None or isinstance(rays, np.ndarray):
            if rays is None:
                records = self.deviceRays()[1]
            else:
                if rays.dtype != _abi.RAY:
                    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
                records = self.uploadRays(rays)
            if records == 0 or records % k:
                raise ValueError("%d uploaded records are not whole sets of %d" % (records, k))
            ptr, n, _keep = None, records // k, None
        else:
            n = _abi.check_ray_sets(rays, k)
            ptr, _keep = C.c_void_p(rays.data_ptr()), rays
        return ptr, n, k, _keep

    def renderRaySets(self, rays, set_size, first_sample, n_samples, out=None):
        """Samples first..first+n-1 of every ray through its SET of set_size records (rt_render_ray_sets, asynchronous):
        sample s of ray i starts at record s mod set_size of ray i's set — anti-aliasing and depth of field for any
        projection (rays.ray_sets, rays.thin_lens make the sets).  `rays`: a torch device tensor (n_rays * set_size, 8) or
        (n_rays, set_size, 8) float32 holding rt_ray bits ray-major, read in place; None: the uploaded records; a numpy
        batch ((n_rays, set_size) _abi.RAY, or float32 of the shapes above) is uploaded first.  `out` as renderRays: an
        (n_rays, 4) device tensor the sums and counts are ADDED to, None: the accumulator (n_rays == w * h)."""
        ptr, n, k, _keep = self._ray_set_args(rays, set_size)
        target = None
        if out is not None:
            _abi.check_ray_target(out, n)
            target = C.c_void_p(out.data_ptr())
        self._check(self._lib.rt_render_ray_sets(self._ctx, ptr, n, k, int(first_sample), int(n_samples), target))

    def renderFeaturesRays(self, rays, follow=0, max_chain=0):
        """Feature records for a w * h batch of rays, ray i = pixel i (rt_render_features_rays, asynchronous): what
        renderFeaturesChain writes for a camera with these primary rays (follow 0: first hits).  `rays` as renderRays.
        Replaces the feature records: the denoisers then work on a frame made by renderRays."""
        ptr, n, _keep = self._ray_args(rays)
        p = _abi.FeatureChainParams(int(follow), int(max_chain))
        self._check(self._lib.rt_render_features_rays(self._ctx, ptr, n, C.byref(p)))

    # -- ray queries: nearest hit and occlusion for any batch; the context's state stays as it is ---------------------------
    def intersectRays(self, rays, follow=0, max_chain=0, out=None):
        """Nearest-hit records for ANY batch of rays (rt_intersect_rays, asynchronous): record i is what renderFeaturesRays
        / renderFeaturesChain would write for ray i (follow 0: first hits), into the caller's buffer — the context's own
        feature records do not move.  `rays` as renderRays.  `out`: an (n, 20) float32 device tensor (n rt_feature
        records), made here if None.  → that tensor; _abi.feature_records(t) gives the (n,) FEATURE records after a sync."""
        import torch
        ptr, n, _keep = self._ray_args(rays)
        if out is None:
            out = torch.empty((n, _abi.FEATURE_FLOATS), dtype=torch.float32, device="cuda:%d" % self._device)
            torch.cuda.synchronize(out.device)
        _abi.check_feature_target(out, n)
        p = _abi.FeatureChainParams(int(follow), int(max_chain))
        self._check(self._lib.rt_intersect_rays(self._ctx, ptr, n, C.byref(p), C.c_void_p(out.data_ptr())))
        return out

    def occludedRays(self, rays, set_size=1, t_max=float("inf"), bounds=None, out=None):
        """Occlusion (any hit) for n sets of set_size records (rt_occluded_rays, asynchronous): a record is occluded iff
        its first hit's t is below its bound — bounds[k] (a float32 device tensor with one float per record, read in place:
        the caller keeps it alive and unchanged until the call has run), or t_max for every record.  `rays` as renderRaySets
        (set_size 1: as renderRays).
        `out`: an (n,) int32 device tensor, made here if None; OVERWRITTEN with the number of occluded records per set.
        → that tensor."""
        import torch
        ptr, n, k, _keep = self._ray_set_args(rays, set_size)
        dev = "cuda:%d" % self._device
        if bounds is not None:
            _abi.check_ray_bounds(bounds, n * k)
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(out.device)
        _abi.check_count_target(out, n)
        self._check(self._lib.rt_occluded_rays(self._ctx, ptr, n, k, C.c_void_p(bounds.data_ptr()) if bounds is not None else None,
                                               float(t_max), C.c_void_p(out.data_ptr())))
        return out

    # -- hemisphere queries: the rays of ambient occlusion and of bakes from hit points, made on the device --------------------
    def _hemispheres(self, features, k, seed, offset, t_max, face_forward, counts, rays_out, want_counts, want_rays):
        import torch
        n = self.width * self.height if features is None else (int(features.shape[0]) if hasattr(features, "shape") and len(features.shape) else 0)
        flags = _abi.HEMI_FACE_FORWARD if face_forward else 0
        dev = "cuda:%d" % self._device
        made = False
        if want_counts and counts is None:
            counts, made = torch.empty((max(n, 0),), dtype=torch.int32, device=dev), True
        if want_rays and rays_out is None and 1 <= int(k) <= _abi.RAY_SET_MAX and 1 <= n * int(k) <= _abi.MAX_RAY_RECORDS:
            rays_out, made = torch.empty((n * int(k), 8), dtype=torch.float32, device=dev), True
        if made:
            torch.cuda.synchronize(torch.device(dev))
        k, flags = _abi.check_hemispheres(features, n, k, flags, offset, counts, rays_out, self.width, self.height,
                                          getattr(self, "_world", 1))
        p = _abi.HemisphereParams(k, flags, int(seed) & 0xFFFFFFFFFFFFFFFF, float(offset), float(t_max))
        self._check(self._lib.rt_occluded_hemispheres(
            self._ctx, C.c_void_p(features.data_ptr()) if features is not None else None, n, C.byref(p),
            C.c_void_p(counts.data_ptr()) if counts is not None else None,
            C.c_void_p(rays_out.data_ptr()) if rays_out is not None else None))
        return counts, rays_out

    def occludedHemispheres(self, features=None, k=16, seed=0, offset=0.0, t_max=float("inf"), face_forward=False, out=None,
                            rays_out=None):
        """How many of k cosine-weighted rays about each record's normal are occluded (rt_occluded_hemispheres,
        asynchronous): the rays are made on the device in registers — rays.hemisphere_sets' rays, in float32 — from
        `features`, an (n, 20) float32 device tensor of rt_feature records (intersectRays' output), or None: the context's
        own width x height records.  A ray is occluded iff its first hit's t is below t_max (occludedRays' rule); a record
        without a hit or with a zero or non-finite normal counts 0.  face_forward: about -normal where the normal looks
        along the record's direction.  `out`: an (n,) int32 device tensor, made here if None, OVERWRITTEN.  `rays_out`: an
        (n * k, 8) or (n, k, 8) float32 device tensor that receives the rays as well (zero bytes for a record without a
        hemisphere).  → out."""
        return self._hemispheres(features, k, seed, offset, t_max, face_forward, out, rays_out, True, False)[0]

    def spawnHemispheres(self, features=None, k=16, seed=0, offset=0.0, face_forward=False, out=None):
        """The rays occludedHemispheres would ask about, without the search (rt_occluded_hemispheres with no counts,
        asynchronous) → an (n * k, 8) float32 device tensor of rt_ray bits, ray-major (`out`, made here if None): it goes
        straight into renderRaySets / occludedRays with set_size k.  The records of a feature record without a hemisphere
        are zero bytes, not rays."""
        return self._hemispheres(features, k, seed, offset, float("inf"), face_forward, None, out, False, True)[1]

    def ambientOcclusion(self, k=16, distance=float("inf"), seed=0, offset=0.0):
        """Ambient occlusion of the context's feature records (renderFeatures & co. made them) → an (h, w) float32 device
        tensor 1 - count / k, 1 where the pixel missed: k rays per pixel about the normal turned to face the viewer,
        occluded by anything nearer than `distance` (occludedHemispheres(None, k, seed, offset, distance, True))."""
        counts = self.occludedHemispheres(None, k, seed, offset, distance, True)
        self.sync()   # (the division runs on torch's stream)
        return (1.0 - counts.float() / float(int(k))).reshape(self.height, self.width)

    def renderHemispheres(self, features=None, k=16, first_sample=0, n_samples=None, seed=0, offset=0.0, face_forward=False,
                          out=None):
        """Hemisphere gather (rt_render_hemispheres, asynchronous): radiance along the k cosine-weighted rays of every
        record — spawnHemispheres' rays, made in registers and never stored — ADDED to `out` exactly as
        renderRaySets(spawnHemispheres(...), k, first_sample, n_samples, out) adds it: sample s of record i follows hemisphere
        ray s mod k.  `features` as occludedHemispheres; n_samples None: k, every ray once.  `out`: an (n, 4) float32 device
        tensor of sums and counts, or None: the accumulator (the context's own frame of records: resolve, the denoisers and
        the moments follow).  A record without a hemisphere adds nothing, its count included.  out.rgb / out.w is the mean
        incoming radiance under the cosine density: irradiance is pi times it.  → out."""
        n = self.width * self.height if features is None else (int(features.shape[0]) if hasattr(features, "shape") and len(features.shape) else 0)
        k, flags, first, count = _abi.check_gather(features, n, k, _abi.HEMI_FACE_FORWARD if face_forward else 0, offset, first_sample,
                                                   n_samples, out, self.width, self.height, getattr(self, "_world", 1))
        p = _abi.HemisphereParams(k, flags, int(seed) & 0xFFFFFFFFFFFFFFFF, float(offset), float("inf"))
        self._check(self._lib.rt_render_hemispheres(
            self._ctx, C.c_void_p(features.data_ptr()) if features is not None else None, n, C.byref(p), first, count,
            C.c_void_p(out.data_ptr()) if out is not None else None))
        return out

    def irradiance(self, k, spp_per_direction=1, seed=0, offset=1e-3):
        """Irradiance at the context's feature records (renderFeatures & co. made them) → an (h, w, 3) float32 device tensor
        pi * rgb / count of renderHemispheres(None, k, 0, k * spp_per_direction, seed, offset, True) into a zeroed target:
        k directions per pixel about the normal turned to face the viewer, each followed spp_per_direction times; 0 where
        the pixel missed."""
        import torch
        k, spp = int(k), int(spp_per_direction)
        if spp < 1:
            raise ValueError("spp_per_direction must be at least 1, not %d" % spp)
        _abi.check_gather(None, self.width * self.height, k, _abi.HEMI_FACE_FORWARD, offset, 0, k * spp, None, self.width, self.height,
                          getattr(self, "_world", 1))
        acc = torch.zeros((self.width * self.height, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        torch.cuda.synchronize(acc.device)
        self.renderHemispheres(None, k, 0, k * spp, seed, offset, True, acc)
        self.sync()   # (the division runs on torch's stream)
        count = acc[:, 3:4]
        # the binary32 quotient, correctly rounded: formed in binary64 and rounded once more (53 >= 2 * 24 + 2 bits)
        mean_pi = ((acc[:, :3] * float(np.float32(np.pi))).double() / count.double()).float()
        return torch.where(count > 0, mean_pi, torch.zeros_like(mean_pi)).reshape(self.height, self.width, 3)

    def lastRayPlan(self):
        """(facts, plan) dicts of the last renderRays / renderRaySets / renderHemispheres launch (rt_debug_last_ray_plan): the camera planner's, with
        n = the rays of the launch's last range."""
        f, p = _abi.CameraFacts(), _abi.CameraPlan()
        self._check(self._lib.rt_debug_last_ray_plan(self._ctx, C.byref(f), C.byref(p)))
        return f.as_dict(), p.as_dict()

    def resolve(self):
        self._check(self._lib.rt_resolve(self._ctx))

    def sync(self):
        self._check(self._lib.rt_sync(self._ctx))

    def renderFrame(self, camera, spp):
        """clear + fused render of samples 0..spp-1 + resolve + sync → gamma image (h,w,4)."""
        self.clear()
        self.renderSamples(camera, 0, spp)
        self.resolve()
        return self.transferImage()

    def renderFrameOnDevice(self, camera, spp):
        """clear + fused render + resolve, all enqueued, nothing read back (the image stays in HBM)."""
        self.clear()
        self.renderSamples(camera, 0, spp)
        self.resolve()

    def renderAdaptive(self, camera, threshold, batch=64, min_spp=128, max_spp=1024, block=(8, 8)):
        """Adaptive frame (rt_render_adaptive): rounds of `batch` samples per pixel until every block of block[0] x
        block[1] pixels has converged (error < threshold, after at least min_spp samples) or holds max_spp samples.
        The image and the linear accumulator are left resolved, as renderFrameOnDevice leaves them.  → stats dict."""
        p = _abi.AdaptiveParams(int(batch), int(min_spp), int(max_spp), float(threshold), int(block[0]), int(block[1]))
        st = _abi.AdaptiveStats()
        self._check(self._lib.rt_render_adaptive(self._ctx, _cam_block(camera).ctypes.data, C.byref(p), C.byref(st)))
        self._adaptive_block = (int(block[0]), int(block[1]))
        return st.as_dict()

    def renderAdaptiveCameras(self, blocks, threshold, batch=64, min_spp=128, block=(8, 8)):
        """Adaptive frame through per-sample camera blocks (rt_render_adaptive_cameras): renderAdaptive with sample j of
        every pixel looking through blocks[j] (float32[max_spp, 12], e.g. Camera.sampleBlocks — pixel jitter, depth of
        field); max_spp = len(blocks).  Each round adds what renderSamplesCameras(blocks[first:first + c], first) adds;
        identical blocks give renderAdaptive's bits.  → the stats dict renderAdaptive returns."""
        blocks = _cam_blocks(blocks)
        p = _abi.AdaptiveParams(int(batch), int(min_spp), len(blocks), float(threshold), int(block[0]), int(block[1]))
        st = _abi.AdaptiveStats()
        self._check(self._lib.rt_render_adaptive_cameras(self._ctx, blocks.ctypes.data if len(blocks) else None, len(blocks),
                                                         C.byref(p), C.byref(st)))
        self._adaptive_block = (int(block[0]), int(block[1]))
        return st.as_dict()

    def renderAdaptiveVariance(self, camera, threshold, batch=16, min_spp=32, max_spp=1024, block=(8, 8)):
        """Adaptive frame under the variance-driven stopping rule (rt_render_adaptive_variance): renderAdaptive's rounds,
        but a block stops once the mean over its pixels of sqrt(M2 / (n (n - 1))) / sqrt(luminance) — the standard error
        of the pixel's mean, measured from its own samples — is below `threshold` (after at least min_spp samples, which
        may equal batch; decisions from round 0 on).  Needs OPT_MOMENTS 1; denoiseMoments can follow directly.
        → the stats dict renderAdaptive returns; pixelError() and blockError() read the estimates."""
        p = _abi.AdaptiveParams(int(batch), int(min_spp), int(max_spp), float(threshold), int(block[0]), int(block[1]))
        st = _abi.AdaptiveStats()
        self._check(self._lib.rt_render_adaptive_variance(self._ctx, _cam_block(camera).ctypes.data, C.byref(p), C.byref(st)))
        self._adaptive_block = (int(block[0]), int(block[1]))
        return st.as_dict()

    def renderAdaptiveVarianceCameras(self, blocks, threshold, batch=16, min_spp=32, block=(8, 8)):
        """renderAdaptiveVariance through per-sample camera blocks (rt_render_adaptive_variance_cameras): sample j of every
        pixel looks through blocks[j] (float32[max_spp, 12]); max_spp = len(blocks).  Identical blocks give
        renderAdaptiveVariance's bits.  → the stats dict renderAdaptive returns."""
        blocks = _cam_blocks(blocks)
        p = _abi.AdaptiveParams(int(batch), int(min_spp), len(blocks), float(threshold), int(block[0]), int(block[1]))
        st = _abi.AdaptiveStats()
        self._check(self._lib.rt_render_adaptive_variance_cameras(self._ctx, blocks.ctypes.data if len(blocks) else None,
                                                                  len(blocks), C.byref(p), C.byref(st)))
        self._adaptive_block = (int(block[0]), int(block[1]))
        return st.as_dict()

    def _adaptive_rays(self, fn, rays, threshold, set_size, batch, min_spp, max_spp, block):
        k = _abi.check_adaptive_set_size(set_size)
        if rays is None or isinstance(rays, np.ndarray):
            if rays is None:
                records = self.deviceRays()[1]
            else:
                if rays.dtype != _abi.RAY:
                    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
                records = self.uploadRays(rays)
            if records == 0 or records % max(k, 1):
                raise ValueError("%d uploaded records are not whole sets of %d" % (records, k))
            ptr, n, _keep = None, records // max(k, 1), None
            if n != self.width * self.height:
                raise ValueError("an adaptive frame takes one ray per pixel: %d rays for %d x %d" % (n, self.width, self.height))
        else:
            n = _abi.check_adaptive_rays(rays, k, self.width, self.height)
            ptr, _keep = C.c_void_p(rays.data_ptr()), rays
        p = _abi.AdaptiveParams(int(batch), int(min_spp), int(max_spp), float(threshold), int(block[0]), int(block[1]))
        st = _abi.AdaptiveStats()
        self._check(fn(self._ctx, ptr, n, k, C.byref(p), C.byref(st)))
        self._adaptive_block = (int(block[0]), int(block[1]))
        return st.as_dict()

    def renderAdaptiveRays(self, rays, threshold, set_size=0, batch=64, min_spp=128, max_spp=1024, block=(8, 8)):
        """Adaptive frame of caller-supplied rays (rt_render_adaptive_rays): renderAdaptive's rounds, stopping rule and
        stats for a w * h batch, ray i = pixel i — a panorama, a fisheye or orthographic view.  `rays` as renderRays
        (set_size 0: one record per ray) or as renderRaySets (set_size 1 .. 4096: ray-major sets, sample s along record
        s mod set_size): a torch device tensor read in place, None for the uploaded records, a numpy batch is uploaded
        first.  Each round adds what renderRays / renderRaySets(first, c) adds to the pixels of the still-active blocks.
        → the stats dict renderAdaptive returns."""
        return self._adaptive_rays(self._lib.rt_render_adaptive_rays, rays, threshold, set_size, batch, min_spp, max_spp, block)

    def renderAdaptiveVarianceRays(self, rays, threshold, set_size=0, batch=16, min_spp=32, max_spp=1024, block=(8, 8)):
        """renderAdaptiveRays under the variance-driven stopping rule (rt_render_adaptive_variance_rays): the rule, the
        parameters and the defaults of renderAdaptiveVariance.  Needs OPT_MOMENTS 1; pixelError() and blockError() read the
        estimates, and denoiseMoments can follow directly.  → the stats dict renderAdaptive returns."""
        return self._adaptive_rays(self._lib.rt_render_adaptive_variance_rays, rays, threshold, set_size, batch, min_spp, max_spp, block)

    def pixelError(self):
        """Pixel errors of the last renderAdaptiveVariance(Cameras / Rays) call (rt_read_pixel_error): each pixel's value after
        the last round its block was traced in → (h, w) float32."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        self._check(self._lib.rt_read_pixel_error(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def devicePixelError(self):
        """Device address of the W x H floats of pixelError() (rt_device_pixel_error)."""
        p = C.c_void_p()
        self._check(self._lib.rt_device_pixel_error(self._ctx, C.byref(p)))
        return p.value

    def sampleCounts(self):
        """Per-pixel sample counts of the accumulator → (h, w) uint32."""
        out = np.empty((self.height, self.width), dtype=np.uint32)
        self._check(self._lib.rt_read_sample_counts(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def blockError(self):
        """Block errors of the last adaptive call, of either stopping rule → (ceil(h/bh), ceil(w/bw)) float32."""
        bw, bh = getattr(self, "_adaptive_block", (8, 8))
        out = np.empty((-(-self.height // bh), -(-self.width // bw)), dtype=np.float32)
        self._check(self._lib.rt_read_block_error(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def renderFeatures(self, camera):
        """First-hit feature records of every pixel for `camera` (rt_render_features, asynchronous).  Leaves the image,
        the accumulator and the sample counter untouched."""
        self._check(self._lib.rt_render_features(self._ctx, _cam_block(camera).ctypes.data))

    def renderFeaturesChain(self, camera, follow=FOLLOW_ALL, max_chain=_abi.FEATURE_CHAIN_MAX):
        """Feature records at the end of every pixel's mirror / glass chain (rt_render_features_chain, asynchronous):
        hits whose material type is in `follow` (FOLLOW_* bits) are followed, at most `max_chain` of them, and the first
        hit that is not is recorded.  Replaces the feature records: featureRecords(), features() and the denoisers
        then work on these.  follow 0 or max_chain 0: renderFeatures."""
        p = _abi.FeatureChainParams(int(follow), int(max_chain))
        self._check(self._lib.rt_render_features_chain(self._ctx, _cam_block(camera).ctypes.data, C.byref(p)))

    def renderFeaturesCameras(self, blocks, follow=0, max_chain=0):
        """Feature records through per-sample cameras (rt_render_features_cameras, asynchronous): the records of the
        n <= 64 camera blocks `blocks` (float32[n, 12], e.g. Camera.sampleBlocks — the guides that belong to a
        renderFrameCameras frame) reduced to one record per pixel: the discrete fields of the dominant (object, chain)
        group, position, depth, normal and albedo averaged over the hit samples, FEATURE_MIXED where the samples disagree.
        `follow` / `max_chain` as renderFeaturesChain (0, 0: first hits).  Replaces the feature records and makes
        featureCoverage()."""
        blocks = _cam_blocks(blocks)
        p = _abi.FeatureChainParams(int(follow), int(max_chain))
        self._check(self._lib.rt_render_features_cameras(self._ctx, blocks.ctypes.data if len(blocks) else None, len(blocks),
                                                         C.byref(p)))

    def featureCoverage(self):
        """The last renderFeaturesCameras call's coverage → (h, w, 2) float32: the share of the samples that hit (the
        anti-aliased alpha) and the share in the dominant group (rt_read_feature_coverage)."""
        out = np.empty((self.height, self.width, 2), dtype=np.float32)
        self._check(self._lib.rt_read_feature_coverage(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def deviceFeatureCoverage(self):
        """Device address of the W x H x 2 coverage floats (rt_device_feature_coverage)."""
        p = C.c_void_p()
        self._check(self._lib.rt_device_feature_coverage(self._ctx, C.byref(p)))
        return p.value

    def featureRecords(self):
        """The last renderFeatures / renderFeaturesChain call's records → (h, w) array of _abi.FEATURE."""
        out = np.empty((self.height, self.width), dtype=_abi.FEATURE)
        self._check(self._lib.rt_read_features(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def features(self):
        """The last renderFeatures call's records as (h, w, ...) arrays: position, depth (t, +inf on a miss), normal,
        albedo, object (kind << 30 | index), material, face, direction, uv, texture, hit; after renderFeaturesChain
        also chain_length, chain_signature (the signature's upper half), cut and chain_word (flags >> 8)."""
        return _abi.split_features(self.featureRecords())

    def denoise(self, camera=None, iterations=_abi.DENOISE_DEFAULTS["iterations"],
                sigma_color=_abi.DENOISE_DEFAULTS["sigma_color"], sigma_normal=_abi.DENOISE_DEFAULTS["sigma_normal"],
                sigma_position=_abi.DENOISE_DEFAULTS["sigma_position"],
                sigma_albedo=_abi.DENOISE_DEFAULTS["sigma_albedo"], split_objects=True, split_chains=False):
        """Edge-avoiding à-trous filter of the linear accumulator guided by the feature records (rt_denoise); renders
        the features for `camera` first when one is given.  → the denoised gamma image (h, w, 4)."""
        if camera is not None:
            self.renderFeatures(camera)
        self.denoiseOnDevice(iterations, sigma_color, sigma_normal, sigma_position, sigma_albedo, split_objects, split_chains)
        return self.denoisedImage()

    def denoiseOnDevice(self, iterations=_abi.DENOISE_DEFAULTS["iterations"],
                        sigma_color=_abi.DENOISE_DEFAULTS["sigma_color"],
                        sigma_normal=_abi.DENOISE_DEFAULTS["sigma_normal"],
                        sigma_position=_abi.DENOISE_DEFAULTS["sigma_position"],
                        sigma_albedo=_abi.DENOISE_DEFAULTS["sigma_albedo"], split_objects=True, split_chains=False):
        """rt_denoise enqueued, nothing read back."""
        p = _abi.DenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position),
                               float(sigma_albedo), _abi.denoise_flags(split_objects, split_chains))
        self._check(self._lib.rt_denoise(self._ctx, C.byref(p)))

    def denoisedImage(self):
        """The last denoise result → gamma RGBA (h, w, 4)."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.rt_read_denoised(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def denoiseVariance(self, camera=None, iterations=_abi.DENOISE_VARIANCE_DEFAULTS["iterations"],
                        sigma_luminance=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_luminance"],
                        sigma_normal=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_normal"],
                        sigma_position=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_position"],
                        sigma_albedo=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_albedo"], split_objects=True, split_chains=False):
        """Variance-guided à-trous filter for low sample counts (rt_denoise_variance); renders the features for
        `camera` first when one is given.  → the denoised gamma image (h, w, 4), the buffer denoisedImage() reads."""
        if camera is not None:
            self.renderFeatures(camera)
        self.denoiseVarianceOnDevice(iterations, sigma_luminance, sigma_normal, sigma_position, sigma_albedo,
                                     split_objects, split_chains)
        return self.denoisedImage()

    def denoiseVarianceOnDevice(self, iterations=_abi.DENOISE_VARIANCE_DEFAULTS["iterations"],
                                sigma_luminance=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_luminance"],
                                sigma_normal=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_normal"],
                                sigma_position=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_position"],
                                sigma_albedo=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_albedo"], split_objects=True, split_chains=False):
        """rt_denoise_variance enqueued, nothing read back."""
        p = _abi.DenoiseVarianceParams(int(iterations), float(sigma_luminance), float(sigma_normal),
                                       float(sigma_position), float(sigma_albedo),
                                       _abi.denoise_flags(split_objects, split_chains))
        self._check(self._lib.rt_denoise_variance(self._ctx, C.byref(p)))

    def variance(self, which=0):
        """The last denoiseVariance call's luminance variance → (h, w) float32: which 0 the 7x7 estimate v0, 1 the
        filtered v(L)."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        self._check(self._lib.rt_read_variance(self._ctx, int(which), out.ctypes.data, out.nbytes))
        return out

    def deviceVariance(self, which=0):
        """Device address of the W x H floats of variance(which) (rt_device_variance)."""
        p = C.c_void_p()
        self._check(self._lib.rt_device_variance(self._ctx, int(which), C.byref(p)))
        return p.value

    def moments(self):
        """Per-pixel centred second moment of the sample luminances, M2 = sum (l(s_j) - mean)^2 over the samples the
        accumulator holds (rt_read_moments; OPT_MOMENTS 1, valid from clear / renderAdaptive on) → (h, w) float32."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        self._check(self._lib.rt_read_moments(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def deviceMoments(self):
        """Device address of the W x H floats of moments() (rt_device_moments)."""
        p = C.c_void_p()
        self._check(self._lib.rt_device_moments(self._ctx, C.byref(p)))
        return p.value

    def sampleVariance(self):
        """Measured variance of every pixel's MEAN luminance, M2 / (n (n - 1)); 0 where n < 2 → (h, w) float32."""
        m2 = self.moments().astype(np.float64)
        n = self.sampleCounts().astype(np.float64)
        ok = n >= 2
        return np.where(ok, m2 / np.where(ok, n * (n - 1.0), 1.0), 0.0).astype(np.float32)

    def denoiseMoments(self, camera=None, iterations=_abi.DENOISE_VARIANCE_DEFAULTS["iterations"],
                       sigma_luminance=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_luminance"],
                       sigma_normal=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_normal"],
                       sigma_position=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_position"],
                       sigma_albedo=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_albedo"], split_objects=True, split_chains=False):
        """The variance-guided filter on MEASURED variance (rt_denoise_moments): denoiseVariance with each pixel's own
        sample variance in place of the 7x7 estimate wherever the pixel holds >= 4 samples; needs OPT_MOMENTS 1 since
        the last clear / renderAdaptive.  Renders the features for `camera` first when one is given.  → the denoised
        gamma image (h, w, 4), the buffer denoisedImage() reads; variance(0 / 1) read its v0 and v(L)."""
        if camera is not None:
            self.renderFeatures(camera)
        self.denoiseMomentsOnDevice(iterations, sigma_luminance, sigma_normal, sigma_position, sigma_albedo,
                                    split_objects, split_chains)
        return self.denoisedImage()

    def denoiseMomentsOnDevice(self, iterations=_abi.DENOISE_VARIANCE_DEFAULTS["iterations"],
                               sigma_luminance=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_luminance"],
                               sigma_normal=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_normal"],
                               sigma_position=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_position"],
                               sigma_albedo=_abi.DENOISE_VARIANCE_DEFAULTS["sigma_albedo"], split_objects=True, split_chains=False):
        """rt_denoise_moments enqueued, nothing read back."""
        p = _abi.DenoiseVarianceParams(int(iterations), float(sigma_luminance), float(sigma_normal),
                                       float(sigma_position), float(sigma_albedo),
                                       _abi.denoise_flags(split_objects, split_chains))
        self._check(self._lib.rt_denoise_moments(self._ctx, C.byref(p)))

    def deviceFeatures(self):
        """Device address of the W x H feature records (rt_device_features)."""
        p = C.c_void_p()
        self._check(self._lib.rt_device_features(self._ctx, C.byref(p)))
        return p.value

    def deviceDenoised(self):
        p = C.c_void_p()
        self._check(self._lib.rt_device_denoised(self._ctx, C.byref(p)))
        return DeviceBuffer(p.value, self.height, self.width, self)

    def traceSamples(self, camera, xs, ys, samples):
        xs = np.ascontiguousarray(xs, dtype=np.uint32)
        ys = np.ascontiguousarray(ys, dtype=np.uint32)
        ss = np.ascontiguousarray(samples, dtype=np.uint32)
        out = np.zeros((len(xs), 3), dtype=np.float32)
        self._check(self._lib.rt_trace_samples(self._ctx, _cam_block(camera).ctypes.data, xs.ctypes.data,
                                               ys.ctypes.data, ss.ctypes.data, len(xs), out.ctypes.data))
        return out

    # -- outputs ------------------------------------------------------------------------
    def transferImage(self, screen=None, shader_tex_id=None):
        """The reference binds a GL texture (src/raytracer.cpp:167-174); here the
        gamma-space RGBA32F image comes back as an (h, w, 4) array, row 0 = y 0."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.rt_read_image(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def readLinear(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.rt_read_linear(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def deviceImage(self):
        p = C.c_void_p()
        self._check(self._lib.rt_device_image(self._ctx, C.byref(p)))
        return DeviceBuffer(p.value, self.height, self.width, self)

    def deviceAccum(self):
        p = C.c_void_p()
        self._check(self._lib.rt_device_accum(self._ctx, C.byref(p)))
        return DeviceBuffer(p.value, self.height, self.width, self)

    # -- measurement ----------------------------------------------------------------------
    def enableCounters(self, on=True):
        self._check(self._lib.rt_enable_counters(self._ctx, 1 if on else 0))

    def resetCounters(self):
        self._check(self._lib.rt_reset_counters(self._ctx))

    def counters(self):
        c = _abi.Counters()
        self._check(self._lib.rt_get_counters(self._ctx, C.byref(c)))
        return c

    def debugCounters(self):
        """(BVH nodes entered, sphere tests executed) since resetCounters(), counting build only."""
        out = (C.c_uint64 * 2)()
        self._check(self._lib.rt_get_debug_counters(self._ctx, out))
        return int(out[0]), int(out[1])

    def walkOverflow(self):
        """Sticky PT_OVF_* bits since resetCounters(): a BVH walk that ended on its loop bound (must be 0)."""
        out = C.c_uint32()
        self._check(self._lib.rt_walk_overflow(self._ctx, C.byref(out)))
        return int(out.value)

    def prefixCacheStats(self):
        """(hits, misses): fused launches that reused the kept prefix (OPT_PREFIX_CACHE) / traced it in full."""
        hits, misses = C.c_uint64(), C.c_uint64()
        self._check(self._lib.rt_prefix_cache_stats(self._ctx, C.byref(hits), C.byref(misses)))
        return int(hits.value), int(misses.value)

    def accumStoreStats(self):
        """(stored, materialised): clear() calls recorded under OPT_ACCUM_STORE 1 that a fused launch ended by storing its
        sums / that ended in the memset, enqueued in front of whatever came next."""
        stored, mat = C.c_uint64(), C.c_uint64()
        self._check(self._lib.rt_accum_store_stats(self._ctx, C.byref(stored), C.byref(mat)))
        return int(stored.value), int(mat.value)

    def lookaheadStats(self):
        """(batches, served, direct, discarded) of renderAgain since the context was made (OPT_LOOKAHEAD): look-ahead
        launches, calls served from a look-ahead frame, calls that ran the direct kernel, frames computed and dropped."""
        v = [C.c_uint64() for _ in range(4)]
        self._check(self._lib.rt_lookahead_stats(self._ctx, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    lookaheadPlan = staticmethod(lookahead_plan)

    def sampleGridStats(self):
        """(launches, exact, workgroups, live_last) of the fused calls' sample kernels since the context was made
        (OPT_EXACT_GRID): launches, those sized by the known length of the live list, workgroups launched in all, and the
        workgroups — all of them with a pixel — of the last exact launch."""
        v = [C.c_uint64() for _ in range(4)]
        self._check(self._lib.rt_sample_grid_stats(self._ctx, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    sampleUnits = staticmethod(sample_units)

    def liveList(self):
        """(seg_cap, pixels per unit, light count, heavy count) of the last fused launch's sample kernel, the counts
        read from the device (rt_debug_live_list; test instrumentation, synchronises)."""
        out = (C.c_uint32 * 4)()
        self._check(self._lib.rt_debug_live_list(self._ctx, out))
        return tuple(int(v) for v in out)

    def waveFixedStats(self):
        """(count64 launches, stage block builds) since the context was made (rt_debug_wave_fixed; test instrumentation):
        fused launches whose sample stage ran the 64-samples-per-pixel instantiation of pt_samples_q, and builds of the
        staged scene block."""
        out = (C.c_uint64 * 2)()
        self._check(self._lib.rt_debug_wave_fixed(self._ctx, out))
        return tuple(int(v) for v in out)

    planSamples = staticmethod(plan_samples)
    planCameraSamples = staticmethod(plan_camera_samples)
    planFeatureCameras = staticmethod(plan_feature_cameras)

    def lastSamplePlan(self):
        """(facts, plan) of the last fused launch's sample stage, as dicts of the fields of _abi.SampleFacts and
        _abi.SamplePlan (rt_debug_last_sample_plan; test instrumentation)."""
        f, p = _abi.SampleFacts(), _abi.SamplePlan()
        self._check(self._lib.rt_debug_last_sample_plan(self._ctx, C.byref(f), C.byref(p)))
        return f.as_dict(), p.as_dict()

    def queueOccupancy(self, lds_bytes):
        """Resident workgroups per compute unit the runtime reports for the headline sample-queue kernel at `lds_bytes` of
        dynamic LDS (rt_debug_queue_occupancy; no kernel runs)."""
        n = C.c_int()
        self._check(self._lib.rt_debug_queue_occupancy(self._ctx, int(lds_bytes), C.byref(n)))
        return int(n.value)

    def stageBlock(self):
        """The staged scene block as it lies on the device, (n, 4) float32 (rt_debug_stage_block; test instrumentation,
        synchronises): the LDS tables the sample queue copies — _abi.stage_block_layout names the rows."""
        cap = 2 * 64 + 2 * 64 + 16
        out = np.zeros((cap, 4), dtype=np.float32)
        n = C.c_uint32()
        self._check(self._lib.rt_debug_stage_block(self._ctx, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].copy()

    def setArith(self, arith):
        """Select the arithmetic policy of the trace kernels (RT_OPT_ARITH): ARITH_IEEE (default, the CPU oracle's
        contract), ARITH_ROCM_OCL_NOCONTRACT or ARITH_ROCM_OCL (the reference as ROCm's OpenCL builds it); a name of
        ARITH_NAMES is accepted too."""
        if isinstance(arith, str):
            arith = ARITH_NAMES[arith]
        self.setOption(OPT_ARITH, int(arith))
        self.arith = int(arith)

    def lastKernelMs(self):
        ms = C.c_float()
        self._check(self._lib.rt_last_kernel_ms(self._ctx, C.byref(ms)))
        return ms.value

    def kernelMsHistory(self, n=64):
        """Device durations (ms) of the last <= min(n, 64) render launches, oldest first."""
        buf = (C.c_float * n)()
        got = C.c_size_t()
        self._check(self._lib.rt_kernel_ms_history(self._ctx, buf, n, C.byref(got)))
        return [buf[i] for i in range(got.value)]

    def stageMsHistory(self, n=64):
        """(first-stage ms, second-stage ms) of the last <= min(n, 64) render launches, oldest first: pt_prefix (or, on a
        call that reuses the kept prefix, pt_final_replay) and the per-sample kernel of a fused call."""
        a, b = (C.c_float * n)(), (C.c_float * n)()
        got = C.c_size_t()
        self._check(self._lib.rt_stage_ms_history(self._ctx, a, b, n, C.byref(got)))
        return [a[i] for i in range(got.value)], [b[i] for i in range(got.value)]

    # -- unit probes of the device routines (tests) -------------------------------------
    def debugHit(self, kind, rays, prim=None, face=None):
        """kind 0 sphere, 1 plane, 2 lens, 3 scene, 4 triangle (mesh prim[i], face[i]) → n × 12 floats (rt_debug_hit)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = len(rays)
        prim = np.zeros(n, np.uint32) if prim is None else np.ascontiguousarray(prim, dtype=np.uint32)
        face = np.zeros(n, np.uint32) if face is None else np.ascontiguousarray(face, dtype=np.uint32)
        out = np.zeros((n, 12), dtype=np.float32)
        self._check(self._lib.rt_debug_hit(self._ctx, kind, rays.ctypes.data, prim.ctypes.data, face.ctypes.data, n,
                                           out.ctypes.data))
        return out

    def debugMaterial(self, routine, vec):
        """routine 0 rayReflect, 1 rayRefract, 2 rayScatter, 3 rayRefractDielectric on n × 16 records → n × 9 floats."""
        vec = np.ascontiguousarray(vec, dtype=np.float32).reshape(-1, 16)
        out = np.zeros((len(vec), 9), dtype=np.float32)
        self._check(self._lib.rt_debug_material(self._ctx, routine, vec.ctypes.data, len(vec), out.ctypes.data))
        return out

    def debugBuiltin(self, op, vec):
        """One builtin of the selected arithmetic policy per record (rt_debug_builtin): n × 8 floats → n × 4 floats.
        Ops 10 and 11 are sqrt and normalize in the tagged forms of the sample queue: a wave is 64 consecutive records.
        Op 12 is min in its tagged form (op 6: the untagged one)."""
        vec = np.ascontiguousarray(vec, dtype=np.float32).reshape(-1, 8)
        out = np.zeros((len(vec), 4), dtype=np.float32)
        self._check(self._lib.rt_debug_builtin(self._ctx, op, vec.ctypes.data, len(vec), out.ctypes.data))
        return out

    def debugDiv3(self, vec):
        vec = np.ascontiguousarray(vec, dtype=np.float32).reshape(-1, 4)
        out = np.zeros((len(vec), 6), dtype=np.float32)
        self._check(self._lib.rt_debug_div3(self._ctx, vec.ctypes.data, len(vec), out.ctypes.data))
        return out

    def debugQueueSums(self, slots, group_log2):
        """One wave's queue_sums (rt_debug_queue_sums): slots (npix, count, 3) float32 → (npix, 4) {sum.rgb, count}."""
        slots = np.ascontiguousarray(slots, dtype=np.float32)
        npix, count = slots.shape[0], slots.shape[1]
        out = np.zeros((npix, 4), dtype=np.float32)
        self._check(self._lib.rt_debug_queue_sums(self._ctx, slots.ctypes.data, npix, count, group_log2, out.ctypes.data))
        return out

    def deviceInfo(self):
        name, arch, cu = C.create_string_buffer(128), C.create_string_buffer(64), C.c_int()
        self._check(self._lib.rt_device_info(self._ctx, name, 128, C.byref(cu), arch, 64))
        return {"name": name.value.decode(), "arch": arch.value.decode(), "cu_count": cu.value}
