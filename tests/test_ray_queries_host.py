"""CPU: the host side of the ray queries (rt_intersect_rays, rt_occluded_rays) — the header and the prototypes, the
refusals of _abi's checks (no device needed), rays.hemisphere_sets and its C++ twin of host/rays.h, the reference helper
tests/ray_queries_ref.py on the CPU oracle (the face-order rule), and the host build: host/ compiles with the façade's two
methods, and a C program that names both functions links against the library."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import ray_queries_ref as Q

rt = cases.rt
A = rt._abi
rays = rt.rays
ROOT = cases.ROOT
GXX = shutil.which("g++") or "g++"
GCC = shutil.which("gcc") or "gcc"
F32 = np.float32


def test_header_symbols_and_prototypes(built):
    header = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert re.search(r"^int rt_intersect_rays\(rt_context \*ctx, const void \*d_rays, size_t n_rays, const rt_feature_chain_params \*p, "
                     r"void \*d_out\);", header, re.M)
    assert re.search(r"^int rt_occluded_rays\(rt_context \*ctx, const void \*d_rays, size_t n_rays, uint32_t set_size, const float \*d_tmax, "
                     r"float t_max,\s+void \*d_out\);", header, re.M)
    assert "rt_intersect_rays" in rt.raytracer.SYMBOLS and "rt_occluded_rays" in rt.raytracer.SYMBOLS
    lib = rt.load_library()
    assert len(lib.rt_intersect_rays.argtypes) == 5 and len(lib.rt_occluded_rays.argtypes) == 7
    assert lib.rt_occluded_rays.argtypes[5] is C.c_float
    assert lib.rt_intersect_rays(None, None, 1, None, None) == -1
    assert lib.rt_occluded_rays(None, None, 1, 1, None, 1.0, None) == -1
    assert hasattr(rt.RayTracer, "intersectRays") and hasattr(rt.RayTracer, "occludedRays")
    for name in ("rt_device_alloc", "rt_device_free", "rt_device_copy"):       # the buffers of a host without a HIP runtime
        assert re.search(r"^int %s\(rt_context \*ctx, " % name, header, re.M) and name in rt.raytracer.SYMBOLS
    assert lib.rt_device_alloc(None, 16, C.byref(C.c_void_p())) == -1 and lib.rt_device_free(None, None) == -1
    assert lib.rt_device_copy(None, None, None, 4, 0) == -1


def test_checks_reject_bad_inputs_without_a_device():
    import torch
    f = torch.zeros((12,), dtype=torch.float32)
    for bad, records in ((np.zeros(12, np.float32), 12), (f.double(), 12), (f, 11), (f.reshape(3, 4), 11), (f.reshape(2, 2, 3), 12),
                         (torch.zeros(24)[::2], 12), (None, 12), (f, 12), (f.reshape(3, 4), 12)):
        with pytest.raises(ValueError):                    # (the last two are fine but for living on the host)
            A.check_ray_bounds(bad, records)
    rec = torch.zeros((6, A.FEATURE_FLOATS), dtype=torch.float32)
    for bad, n in ((np.zeros((6, 20), np.float32), 6), (rec.double(), 6), (rec, 5), (torch.zeros((6, 19)), 6), (torch.zeros(120), 6),
                   (torch.zeros((12, 20))[::2], 6), (None, 6), (rec, 6)):
        with pytest.raises(ValueError):
            A.check_feature_target(bad, n)
    cnt = torch.zeros((6,), dtype=torch.int32)
    for bad, n in ((np.zeros(6, np.int32), 6), (cnt.float(), 6), (cnt.long(), 6), (cnt, 5), (cnt.reshape(2, 3), 6),
                   (torch.zeros(12, dtype=torch.int32)[::2], 6), (None, 6), (cnt, 6)):
        with pytest.raises(ValueError):
            A.check_count_target(bad, n)
    assert A.FEATURE_FLOATS * 4 == A.FEATURE.itemsize
    got = A.feature_records(torch.arange(40, dtype=torch.float32).reshape(2, 20))
    assert got.shape == (2,) and got.dtype == A.FEATURE and got["t"][1] == 23.0 and got["pos"][0, 2] == 2.0


def surface_points(n):
    u = rt.workloads.uniforms(n, 5, cases.SEED).astype(np.float64)
    normals = 2 * u[:, :3] - 1
    normals[:6] = np.concatenate([np.eye(3), -np.eye(3)])              # the axes: the tangent frame's corner cases
    normals[6] = (0.0, 3.0, 0.0)                                       # not unit
    normals[7] = (1e-3, 1.0, 1e-3)
    points = 10 * rt.workloads.uniforms(n, 6, cases.SEED)[:, :3].astype(np.float64) - 5
    return points.astype(F32), normals.astype(F32)


@pytest.mark.parametrize("k", [1, 16])
def test_hemisphere_sets_properties(k):
    points, normals = surface_points(300)
    sets = rays.hemisphere_sets(points, normals, k, 7)
    assert sets.shape == (300, k) and sets.dtype == A.RAY and sets.flags["C_CONTIGUOUS"]
    assert sets.tobytes() == rays.hemisphere_sets(points, normals, k, 7).tobytes()          # deterministic
    assert sets.tobytes() != rays.hemisphere_sets(points, normals, k, 8).tobytes()
    d = sets["d"].astype(np.float64)
    unit = normals.astype(np.float64) / np.linalg.norm(normals.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() <= 1e-6
    cos = (d * unit[:, None, :]).sum(-1)
    assert cos.min() > 0.0
    assert (sets["o"] == points[:, None, :]).all()                     # offset 0: the origin is the point itself
    assert (sets["x"] == np.arange(300)[:, None]).all() and (sets["y"] == 0).all()
    if k == 16:                                                        # cosine-weighted: E[cos] = 2/3, sd 0.236 / sqrt(4800)
        assert abs(cos.mean() - 2.0 / 3.0) < 5 * 0.236 / np.sqrt(cos.size)
        # the azimuth about the normal is uniform: the mean tangential part vanishes (sd <= 1 / sqrt(2 m) per axis)
        tang = d - cos[..., None] * unit[:, None, :]
        assert np.abs(tang.reshape(-1, 3).mean(0)).max() < 5 / np.sqrt(2 * cos.size)
    lifted = rays.hemisphere_sets(points, normals, k, 7, offset=0.25)
    assert np.abs(lifted["o"] - (points + F32(0.25) * unit.astype(F32))[:, None, :]).max() <= 1e-6
    assert lifted["d"].tobytes() == sets["d"].tobytes()
    for bad in (dict(points=points[:-1]), dict(k=0), dict(k=A.RAY_SET_MAX + 1), dict(normals=np.zeros_like(normals))):
        kw = dict(points=points, normals=normals, k=k, seed=7)
        kw.update(bad)
        with pytest.raises(ValueError):
            rays.hemisphere_sets(**kw)


def test_ray_queries_ref_reproduces_the_face_order_rule(oracle):
    scene = Q.face_order_scene()
    assert len(scene.meshes) == 1 and scene.meshes["face_count"][0] == Q.FACE_ORDER_FACES == 36
    ray = Q.FACE_ORDER_RAY[None, :]
    side = np.array([[50, 0, 0, 0, 0, 1]], F32)
    assert Q.first_hit_t(oracle, scene, ray)[0] == F32(6.0)            # the far face: the first in face order
    assert Q.first_hit_t(oracle, scene, side)[0] == F32(5.0)
    assert np.isinf(Q.first_hit_t(oracle, scene, np.array([[0, 5, 0, 0, 0, 1]], F32))[0])
    for bound, want in Q.FACE_ORDER_CASES:
        assert bool(Q.occluded_ref(oracle, scene, ray, F32(bound))[0]) is want
    t = np.array([2.0, np.inf, 0.5, 7.0], F32)
    b = Q.cycled_bounds(np.repeat(t, 12))
    assert b.shape == (48,) and np.isnan(b[6::12]).all() and (b[0:4] == [2.0, np.nextafter(F32(2), F32(3)), np.nextafter(F32(2), F32(0)), 1.0]).all()
    want = np.zeros(12, bool)
    want[[1, 4, 5, 10, 11]] = True                                     # above t, 2 t, +inf, 1000 and the float above it
    assert np.array_equal(Q.occluded(np.repeat(t, 12), b)[:12], want)
    assert not Q.occluded(np.repeat(t, 12), b)[12:24].any()            # a miss is below no bound
    rays6 = Q.box_rays(rt.workloads.get("all_kinds", width=48, height=27).scene, 300, 900)
    assert rays6.shape == (300, 6) and np.abs(np.linalg.norm(rays6[:, 3:].astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ray_queries") / "ray_queries_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "ray_queries_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("k", [1, 16])
def test_cpp_hemisphere_sets_has_the_same_properties(k, program):
    points, normals = surface_points(200)
    stdin = np.concatenate([points, normals], axis=1).astype(F32).tobytes()
    p = subprocess.run([program, str(k), "7", "0.25"], input=stdin, capture_output=True)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()
    got = np.frombuffer(p.stdout, dtype=A.RAY).reshape(200, k)
    assert subprocess.run([program, str(k), "7", "0.25"], input=stdin, capture_output=True).stdout == p.stdout
    d = got["d"].astype(np.float64)
    unit = normals.astype(np.float64) / np.linalg.norm(normals.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() <= 1e-6
    assert (d * unit[:, None, :]).sum(-1).min() > 0.0
    assert (got["x"] == np.arange(200)[:, None]).all() and (got["y"] == 0).all()
    # the same generator and the same formulas: sin / cos may differ in their last place, nothing more
    want = rays.hemisphere_sets(points, normals, k, 7, offset=0.25)
    assert np.abs(got["d"] - want["d"]).max() <= 4e-7 and np.abs(got["o"] - want["o"]).max() <= 1e-6
    assert subprocess.run([program, "0", "7", "0"], input=stdin, capture_output=True).returncode == 3


def test_host_builds_and_a_c_program_links(built, tmp_path):
    assert os.path.isfile(os.path.join(ROOT, "host", "rt_cli")) and os.path.isfile(os.path.join(ROOT, "host", "librt_host.a"))
    header = open(os.path.join(ROOT, "host", "raytracer.h")).read()
    assert "intersectRays(" in header and "occludedRays(" in header
    symbols = subprocess.run(["nm", "-C", os.path.join(ROOT, "host", "librt_host.a")], capture_output=True, text=True, check=True).stdout
    assert "RayTracer::intersectRays(" in symbols and "RayTracer::occludedRays(" in symbols
    p = subprocess.run([os.path.join(ROOT, "host", "rt_cli"), "--scene", "x.scene", "--ao", "4"], capture_output=True, text=True)
    assert p.returncode == 2 and "--ao K" in p.stderr and "32 B x W x H x K" in p.stderr          # --ao goes with --aov
    exe = str(tmp_path / "ray_queries_link")
    libdir = os.path.join(ROOT, "opencl-raytracing_amd")
    subprocess.run([GCC, "-std=c99", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "ray_queries_link.c"), "-o", exe,
                    "-L" + libdir, "-lrt_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["-1", "-1"], (p.stdout, p.stderr)
