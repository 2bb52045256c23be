"""MI355X-native path tracer — host-side Python mirror of the reference's
RayTracer / SceneCreator / Camera API over the C ABI of librt_amd.so
(include/rt_amd.h).  The directory name carries a hyphen; import it with
``import opencl_raytracing_amd`` (repo-root shim) or
``importlib.import_module("opencl-raytracing_amd")``.
"""
from . import _abi, rays, workloads  # noqa: F401
from .camera import Camera  # noqa: F401
from .raytracer import (ARITH_IEEE, ARITH_NAMES, ARITH_ROCM_OCL, ARITH_ROCM_OCL_NOCONTRACT, FOLLOW_ALL,  # noqa: F401
                        FOLLOW_DIELECTRIC, FOLLOW_REFLECTIVE, FOLLOW_REFRACTIVE, LIB_PATH, RayTracer, RtError, check_accel,
                        feature_chain_signature, load_library, lookahead_plan, make_random_table, plan_feature_cameras,
                        sample_units)
from .scene import SceneCreator, SceneError  # noqa: F401

__all__ = ["Camera", "RayTracer", "RtError", "SceneCreator", "SceneError", "workloads", "rays", "load_library",
           "make_random_table", "lookahead_plan", "sample_units", "feature_chain_signature", "plan_feature_cameras",
           "FOLLOW_REFLECTIVE",
           "FOLLOW_REFRACTIVE", "FOLLOW_DIELECTRIC", "FOLLOW_ALL", "LIB_PATH"]
