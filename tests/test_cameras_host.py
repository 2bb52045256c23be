"""CPU: per-sample camera blocks — the header as plain C and the exported symbols, Camera.sampleBlocks in Python and in
C++ (same bits), the properties of its Halton offsets and of its lens, and the camera launcher's plan
(rt_debug_plan_camera_samples, the launcher's own function) against its restatement (tests/camera_plan_ref.py) and
against rows written out by hand."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import cases
import camera_plan_ref as R

rt = cases.rt
ROOT = cases.ROOT
f32 = np.float32
plan_camera_samples = rt.raytracer.plan_camera_samples
FIXED, QUEUE = R.FIXED, R.QUEUE
NEW_SYMBOLS = ("rt_render_spp_cameras", "rt_debug_plan_camera_samples", "rt_debug_last_camera_plan")


def test_header_compiles_as_plain_c_and_the_symbols_are_exported(built, tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "rt_amd.h"\n'
                   "int use(rt_context *c, const float *cams) {\n"
                   "    rt_camera_facts f = {0}; rt_camera_plan p;\n"
                   "    if (rt_debug_plan_camera_samples(&f, &p) != RT_EINVAL) return 1;\n"
                   "    if (rt_debug_last_camera_plan(c, &f, &p)) return 2;\n"
                   "    return rt_render_spp_cameras(c, cams, 0u, 64u) + (int)RT_CAMERA_PLAN_QUEUE + (int)RT_CAMERA_PLAN_FIXED;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)
    lib = rt.load_library()
    for s in NEW_SYMBOLS:
        assert s in rt.raytracer.SYMBOLS and getattr(lib, s)
    assert lib.rt_abi_version() == 3


def _camera():
    return rt.Camera(60, 16.0 / 9.0, pos=(-8.0, -1.0, -8.0), y=45.0, p=-5.0)


def test_with_everything_off_every_block_is_the_camera_block():
    cam = _camera()
    b = cam.sampleBlocks(7, first_sample=3, pixel_jitter=False)
    assert b.shape == (7, 12) and b.dtype == f32
    assert all(np.array_equal(row.view(np.uint32), cam.transferData().view(np.uint32)) for row in b)
    b = cam.sampleBlocks(7, width=64, height=36, pixel_jitter=False, aperture=0.0, focus=8.0)   # (no lens: the focus is not used)
    assert all(np.array_equal(row.view(np.uint32), cam.transferData().view(np.uint32)) for row in b)


DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "camera.h"
int main(int argc, char **argv) {
    if (argc != 8) return 2;
    Camera cam(60, 16.0f / 9.0f, rth::vec3(-8.0f, -1.0f, -8.0f), 45.0f, -5.0f);
    std::vector<float> b = cam.sampleBlocks((uint32_t)atoi(argv[1]), (uint32_t)atoi(argv[2]), atoi(argv[3]), atoi(argv[4]),
                                            atoi(argv[5]) != 0, (float)atof(argv[6]), (float)atof(argv[7]));
    fwrite(b.data(), sizeof(float), b.size(), stdout);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_blocks(tmp_path_factory):
    d = tmp_path_factory.mktemp("blocks")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "host"), str(d / "driver.cpp"),
                    os.path.join(ROOT, "host", "camera.cpp"), "-o", exe], check=True)

    def run(n, first, w, h, jitter, aperture, focus):
        out = subprocess.run([exe, str(n), str(first), str(w), str(h), str(int(jitter)), repr(aperture), repr(focus)],
                             check=True, capture_output=True).stdout
        return np.frombuffer(out, dtype=f32).reshape(n, 12)
    return run


@pytest.mark.parametrize("first", [0, 64])
@pytest.mark.parametrize("jitter,aperture,focus", [(True, 0.0, 1.0), (False, 0.05, 8.0), (True, 0.05, 8.0), (False, 0.0, 1.0)])
def test_cpp_blocks_equal_python_blocks(cpp_blocks, first, jitter, aperture, focus):
    want = _camera().sampleBlocks(64, first_sample=first, width=1920, height=1080, pixel_jitter=jitter, aperture=aperture, focus=focus)
    got = cpp_blocks(64, first, 1920, 1080, jitter, aperture, focus)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_consecutive_calls_continue_one_sequence():
    cam = _camera()
    whole = cam.sampleBlocks(128, width=100, height=60, aperture=0.1, focus=5.0)
    parts = np.concatenate([cam.sampleBlocks(64, first_sample=f, width=100, height=60, aperture=0.1, focus=5.0) for f in (0, 64)])
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    assert len({row.tobytes() for row in whole}) == 128


def test_offsets_are_halton_points_of_a_pixel():
    off = rt.Camera.sampleOffsets(4096)
    assert (off[:, :2] >= -0.5).all() and (off[:, :2] < 0.5).all()
    # the first 64 points of Halton(2) are the odd multiples of 1 / 128 (mean exactly 0.5), those of Halton(3) fill the 81
    # cells of width 1 / 81 at most once: both means are within 1 / 64 of the pixel's centre
    assert np.abs(off[:64, :2].astype(np.float64).mean(0)).max() <= 1.0 / 64.0
    # and they are the offsets sampleBlocks applies: llc' - llc = (dx / w) hor + (dy / h) ver
    cam = _camera()
    b = cam.sampleBlocks(16, width=40, height=30)
    for j in range(16):
        want = cam.lower_left_corner + (off[j, 0] / f32(40)) * cam.horizontal
        want = want + (off[j, 1] / f32(30)) * cam.vertical
        assert np.array_equal(b[j, 3:6].view(np.uint32), want.astype(f32).view(np.uint32))


def test_lens_points_lie_inside_the_unit_disk():
    off = rt.Camera.sampleOffsets(4096).astype(np.float64)
    r2 = off[:, 2] ** 2 + off[:, 3] ** 2
    assert (r2 < 1.0).all() and r2.max() > 0.9 and len(np.unique(off[:, 2:], axis=0)) == 4096


def test_the_focus_plane_stays_where_it_is():
    cam = _camera()
    F = f32(8.0)
    b = cam.sampleBlocks(64, width=64, height=36, pixel_jitter=False, aperture=0.25, focus=float(F)).astype(np.float64)
    pos, llc, hor, ver = (np.asarray(v, dtype=np.float64) for v in (cam.position, cam.lower_left_corner, cam.horizontal, cam.vertical))
    assert np.abs(b[:, 0:3] - pos).max() > 0.05          # the lens points move the origin ...
    for s, t in itertools.product((0.0, 0.5, 1.0), repeat=2):
        want = pos + float(F) * (llc + s * hor + t * ver)
        got = b[:, 0:3] + b[:, 3:6] + s * b[:, 6:9] + t * b[:, 9:12]
        # ... and not the point they look at: float32 rounding of values of magnitude <= |pos| + F |llc + hor + ver| < 40
        assert np.abs(got - want).max() <= 40 * 8 * 2.0 ** -24


# ---- the camera launcher's plan --------------------------------------------------------------------------------------------
GEOMETRY = {   # (lenses, models, faces, spheres, sphere BVH, mesh BVH) → the (ACCEL, GEOM) row of the camera queue
    "spheres": ((0, 0, 0, 8, 0, 0), (0, 0)),
    "lens": ((1, 0, 0, 8, 0, 0), (0, 1)),
    "small_mesh_12": ((0, 1, 12, 8, 0, 0), (0, 1)),
    "small_meshes_65": ((0, 2, 65, 8, 0, 0), (0, 1)),
    "sphere_bvh": ((0, 0, 0, 2000, 1, 0), (1, 0)),
    "sphere_bvh_lens": ((1, 0, 0, 2000, 1, 0), (1, 1)),
    "bvh_mesh": ((0, 1, 1000, 8, 0, 1), (1, 2)),
    "bvh_mesh_sphere_bvh": ((0, 2, 1012, 2000, 1, 1), (1, 2)),
}
COUNTS = [(c, R.group_log2_for(c)) for c in (1, 7, 8, 63, 64, 65, 384, 512)] + [(64, 5)]


def _facts(geometry, count, glog2, n, counters, moments, queue, fill):
    lenses, models, faces, spheres, sphere_bvh, mesh_bvh = GEOMETRY[geometry][0]
    return dict(count=count, glog2=glog2, n=n, material_count=6, sphere_count=spheres, plane_count=1, lens_count=lenses,
                model_count=models, sphere_bvh=sphere_bvh, mesh_bvh=mesh_bvh, faces=faces, cu_count=256, count_enabled=counters,
                sample_queue=queue, wave_fill=fill, moments=moments)


@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_the_camera_plan_equals_its_restatement(built, geometry):
    families = set()
    for (count, glog2), n in itertools.product(COUNTS, (1, 256, 61 * 35, 2073600)):
        for counters, moments, queue, fill in itertools.product((0, 1), repeat=4):
            f = _facts(geometry, count, glog2, n, counters, moments, queue, fill)
            got, want = plan_camera_samples(**f), R.plan(f)
            assert got == want, (f, got, want)
            families.add(got["family"])
            if got["family"] == QUEUE:
                assert not counters and not moments and queue
                assert (got["accel"], got["geom"]) == GEOMETRY[geometry][1]
                assert 1 <= got["pixels_per_wave"] <= 16 and got["pixels_per_wave"] * count <= 512
                assert got["block_size"] == 64 and got["lds_bytes"] <= 65536
                # exact sizing: every slot has a wave, and the last wave has a slot
                assert (got["grid_units"] - 1) * got["pixels_per_wave"] < n <= got["grid_units"] * got["pixels_per_wave"]
            else:
                assert counters or moments or not queue
                assert got["grid_units"] * 256 >= n << glog2 > (got["grid_units"] - 1) * 256
    assert families == {FIXED, QUEUE}


def test_refuses_facts_no_camera_launch_can_have(built):
    f = _facts("spheres", 64, 6, 256, 0, 0, 1, 1)
    for bad in (dict(count=0), dict(count=513), dict(glog2=7)):
        with pytest.raises(rt.RtError):
            plan_camera_samples(**dict(f, **bad))


HD = 1920 * 1080


def _scene(name, **kw):
    return rt.workloads.get(name, width=16, height=16, **kw).scene


def _key(p):
    return (p["family"], bool(p["count"]), bool(p["accel"]), p["geom"], p["waves"], bool(p["moments"]))


def test_hand_written_rows_at_1080p_and_64_samples(built):
    c2 = _scene("c2")
    p = plan_camera_samples(**R.facts_of(c2, HD, 64))
    static = 2 * len(c2.materials) + 2 * len(c2.spheres) + len(c2.planes)
    assert _key(p) == (QUEUE, False, False, 0, 6, False)
    assert (p["pixels_per_wave"], p["grid_units"], p["block_size"]) == (6, HD // 6, 64)      # the fused launch's six pixels per wave
    assert p["lds_bytes"] == 16 * static + 6 * (6 * 16 + 64 * 12) and p["lds_face_f4"] == 0
    # the fixed-lane kernel serves counters, moments and RT_OPT_SAMPLE_QUEUE 0: 64 lanes per pixel, 256 per workgroup
    for other in (dict(count_enabled=1), dict(moments=1), dict(sample_queue=0)):
        q = plan_camera_samples(**R.facts_of(c2, HD, 64, **other))
        assert q["family"] == FIXED and (q["grid_units"], q["block_size"], q["lds_bytes"], q["pixels_per_wave"]) == (HD * 64 // 256, 256, 0, 1)
    c3 = _scene("c3", tex_size=8)
    p = plan_camera_samples(**R.facts_of(c3, HD, 64))
    assert _key(p) == (QUEUE, False, False, 1, 6, False) and p["lds_face_f4"] == 36          # its cube in LDS
    c4 = _scene("c4", n_spheres=2000)
    assert _key(plan_camera_samples(**R.facts_of(c4, HD, 64))) == (QUEUE, False, True, 0, 6, False)
    assert _key(plan_camera_samples(**dict(R.facts_of(c4, HD, 64), lens_count=1))) == (QUEUE, False, True, 1, 5, False)
    assert _key(plan_camera_samples(**R.facts_of(c4, HD, 64, accel=0))) == (QUEUE, False, False, 0, 6, False)
    c5 = _scene("c5", segments=16, rings=10)
    p = plan_camera_samples(**R.facts_of(c5, HD, 64))                                         # a walk-slice scene: the (1, 2) row
    assert _key(p) == (QUEUE, False, True, 2, 5, False) and p["lds_face_f4"] == 0
    # a small frame spreads over the chip, as a fused launch does
    assert plan_camera_samples(**R.facts_of(c2, 200 * 126, 64))["pixels_per_wave"] == 1
    assert plan_camera_samples(**R.facts_of(c2, 200 * 126, 64, wave_fill=0))["pixels_per_wave"] == 6


def test_cli_refuses_per_sample_cameras_with_one_camera_modes(built):
    cli = os.path.join(ROOT, "host", "rt_cli")
    for flags in (["--aa", "--progressive"], ["--aa", "--adaptive", "0.01"], ["--aperture", "0.1", "--focus", "4", "--progressive"]):
        p = subprocess.run([cli] + flags, capture_output=True, text=True, cwd=ROOT)
        assert p.returncode == 2 and "use --spp" in p.stderr, (flags, p.stderr)
    for flags in (["--aperture", "0.1"], ["--focus", "4"], ["--aperture", "-1", "--focus", "4"]):   # a lens has a radius and a focus
        p = subprocess.run([cli] + flags, capture_output=True, text=True, cwd=ROOT)
        assert p.returncode == 2 and "usage" in p.stderr, (flags, p.stderr)
