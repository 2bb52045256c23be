"""CPU: the host side of ray sets (rt_render_ray_sets) — the generators' `offset`, rays.ray_sets, rays.thin_lens,
_abi.check_ray_sets' refusals (no device needed), the kernels' remainder rule restated, and host/rays.h's offsets and
ray_sets through a stand-alone program (tests/host/ray_sets_main.cpp) against the Python generators."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases

rt = cases.rt
A = rt._abi
rays = rt.rays
ROOT = cases.ROOT
GXX = shutil.which("g++") or "g++"
F32_EPS = float(np.finfo(np.float32).eps)
POS = (1.5, -2.25, 0.75)
CAM = rt.Camera(60, np.float32(16) / np.float32(9), (-8, -1, -8), 45.0, 0.0)

GENERATORS = {   # name → (generator, keyword arguments, frame width)
    "equirect": (rays.equirect_rays, dict(pos=POS, w=33, h=17, yaw=20.0), 33),
    "fisheye": (rays.fisheye_rays, dict(pos=POS, w=21, h=15, fov_deg=170.0, yaw=30.0, pitch=-10.0), 21),
    "ortho": (rays.orthographic_rays, dict(pos=POS, w=12, h=7, extent=4.0, yaw=30.0, pitch=-10.0), 12),
    "cubemap": (rays.cubemap_rays, dict(pos=POS, face_size=5), 5),
    "primary": (rays.primary_rays, dict(camera_block=CAM.transferData(), w=16, h=9), 16),
}


def todays_grid(w, h, centre=True):
    """_grid as it stood before `offset` existed"""
    off = 0.5 if centre else 0.0
    s = (np.arange(w, dtype=np.float64) + off) / w
    t = (np.arange(h, dtype=np.float64) + off) / h
    ss, tt = np.meshgrid(s, t)
    return ss.reshape(-1), tt.reshape(-1)


@pytest.mark.parametrize("kind", sorted(GENERATORS))
def test_default_offset_gives_todays_bits(kind, monkeypatch):
    gen, kw, _ = GENERATORS[kind]
    default, zero = gen(**kw), gen(offset=(0.0, 0.0), **kw)
    assert default.tobytes() == zero.tobytes()
    monkeypatch.setattr(rays, "_grid", lambda w, h, centre=True, offset=(0.0, 0.0): todays_grid(int(w), int(h), centre))
    assert gen(**kw).tobytes() == default.tobytes()
    monkeypatch.undo()
    moved = gen(offset=(0.25, -0.25), **kw)
    assert moved.tobytes() != default.tobytes() and np.array_equal(moved["x"], default["x"]) and np.array_equal(moved["y"], default["y"])


def test_an_offset_of_half_a_pixel_is_half_way_to_the_next_centre():
    w, h = 12, 7
    kw = dict(pos=POS, w=w, h=h, extent=4.0, yaw=30.0, pitch=-10.0)
    base = rays.orthographic_rays(**kw).reshape(h, w)
    half = rays.orthographic_rays(offset=(0.5, 0.0), **kw).reshape(h, w)
    full = rays.orthographic_rays(offset=(1.0, 0.0), **kw).reshape(h, w)
    # a whole pixel to the right IS the next pixel's centre, to float32 rounding (the double sums differ in their last place)
    assert np.abs(full["o"][:, :-1] - base["o"][:, 1:]).max() <= 4 * F32_EPS * np.abs(base["o"]).max()
    mid = 0.5 * (base["o"][:, :-1].astype(np.float64) + base["o"][:, 1:])
    assert np.abs(half["o"][:, :-1] - mid).max() <= 4 * F32_EPS * np.abs(base["o"]).max()
    assert (half["d"] == base["d"]).all()
    down = rays.orthographic_rays(offset=(0.0, 1.0), **kw).reshape(h, w)
    assert np.abs(down["o"][:-1] - base["o"][1:]).max() <= 4 * F32_EPS * np.abs(base["o"]).max()
    # primary_rays adds the offset to x and y
    block = CAM.transferData()
    p0 = rays.primary_rays(block, 16, 9).reshape(9, 16)
    p1 = rays.primary_rays(block, 16, 9, offset=(1.0, 0.0)).reshape(9, 16)
    assert np.abs(p1["d"][:, :-1] - p0["d"][:, 1:]).max() <= 2 * F32_EPS


def test_ray_sets_shape_order_and_ids():
    gen, kw, w = GENERATORS["fisheye"]
    k = 6
    offsets = rt.Camera.sampleOffsets(k)
    assert offsets.shape == (k, 4) and (np.abs(offsets[:, :2]) <= 0.5).all()
    sets = rays.ray_sets(gen, offsets, **kw)
    n = kw["w"] * kw["h"]
    assert sets.shape == (n, k) and sets.dtype == A.RAY and sets.flags["C_CONTIGUOUS"]
    for t in range(k):
        col = gen(offset=tuple(offsets[t, :2]), **kw)
        assert sets[:, t]["o"].tobytes() == col["o"].tobytes() and sets[:, t]["d"].tobytes() == col["d"].tobytes()
    i = np.arange(n)
    assert (sets["x"] == (i % w)[:, None]).all() and (sets["y"] == (i // w)[:, None]).all()
    # ray-major in memory: record i * k + t
    flat = rays.as_floats(sets)
    assert flat.shape == (n * k, 8) and flat[3 * k + 2].tobytes() == sets[3, 2].tobytes()
    assert rays.ray_sets(gen, offsets[:, :2], **kw).tobytes() == sets.tobytes()       # (k, 2) offsets are the same thing
    for bad in (offsets[:0], offsets[:, :3], offsets[0], np.zeros((A.RAY_SET_MAX + 1, 2))):
        with pytest.raises(ValueError):
            rays.ray_sets(gen, bad, **kw)


def test_thin_lens_keeps_the_focus_point():
    gen, kw, _ = GENERATORS["equirect"]
    k = 8
    offsets = rt.Camera.sampleOffsets(k)
    sets = rays.ray_sets(gen, offsets, **kw)
    _, U, V = rays.basis(20.0, 0.0)
    focus, aperture = 6.0, 0.25
    out = rays.thin_lens(sets, U, V, aperture, focus, offsets)
    assert out.shape == sets.shape and np.array_equal(out["x"], sets["x"]) and np.array_equal(out["y"], sets["y"])
    o, d = sets["o"].astype(np.float64), sets["d"].astype(np.float64)
    o2, d2 = out["o"].astype(np.float64), out["d"].astype(np.float64)
    target = o + focus * d
    along = ((target - o2) * d2).sum(-1, keepdims=True)                 # the new ray's point nearest the focus point
    assert np.abs(o2 + along * d2 - target).max() <= 1e-5 * focus
    assert np.abs(np.linalg.norm(d2, axis=-1) - 1.0).max() <= 2 * F32_EPS
    shift = np.linalg.norm(o2 - o, axis=-1)
    lens_r = np.linalg.norm(offsets[:, 2:].astype(np.float64), axis=1)
    assert np.abs(shift - aperture * lens_r[None, :]).max() <= 1e-6 and shift.max() > 0.1 * aperture
    # (k, 2) lens points are the same thing; aperture 0 returns the input bits
    assert rays.thin_lens(sets, U, V, aperture, focus, offsets[:, 2:]).tobytes() == out.tobytes()
    assert rays.thin_lens(sets, U, V, 0.0, focus, offsets).tobytes() == sets.tobytes()
    with pytest.raises(ValueError):
        rays.thin_lens(sets, U, V, aperture, focus, offsets[:-1])
    with pytest.raises(ValueError):
        rays.thin_lens(sets[:, 0], U, V, aperture, focus, offsets)


def test_check_ray_sets_rejects_bad_inputs_without_a_device():
    import torch
    good = torch.zeros((12, 8), dtype=torch.float32)
    bad = [(np.zeros((12, 8), np.float32), 4), (good.double(), 4), (torch.zeros((12, 6)), 4), (torch.zeros((96,)), 4),
           (torch.zeros((0, 8)), 4), (good, 5), (good, 0), (good, A.RAY_SET_MAX + 1), (good.reshape(3, 4, 8), 3),
           (good.reshape(3, 4, 8), 2), (torch.zeros((3, 4, 6)), 4), (torch.zeros((24, 8))[::2], 4), (None, 4),
           (good, 4), (good.reshape(3, 4, 8), 4)]
    for b, k in bad:                                # (the last two are fine but for living on the host)
        with pytest.raises(ValueError):
            A.check_ray_sets(b, k)
    assert A.RAY_SET_MAX == 4096
    lib = rt.load_library()
    assert lib.rt_render_ray_sets.argtypes and len(lib.rt_render_ray_sets.argtypes) == 7
    assert lib.rt_render_ray_sets(None, None, 1, 1, 0, 1, None) == -1
    assert hasattr(rt.RayTracer, "renderRaySets")


def test_the_kernels_remainder_rule():
    """ray_set_member (csrc/pt_sample.hpp): s mod k as s - uint(float(s) + 0.5f) * (1.0f / k)) * k, every operation in
    float32, over the whole domain the library admits: samples 0 .. RT_MAX_SAMPLE, set sizes 1 .. RT_RAY_SET_MAX."""
    s = np.arange(0, 65536, dtype=np.uint32)
    sf = s.astype(np.float32) + np.float32(0.5)
    for k in range(1, A.RAY_SET_MAX + 1):
        q = (sf * (np.float32(1.0) / np.float32(k))).astype(np.uint32)
        assert np.array_equal(s - q * np.uint32(k), s % np.uint32(k)), k


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ray_sets") / "ray_sets_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "ray_sets_main.cpp"), "-o", exe], check=True)
    return exe


CPP_CASES = {
    "equirect": ["33", "17", "20"],
    "fisheye": ["21", "15", "170", "30", "-10"],
    "ortho": ["12", "7", "4", "30", "-10"],
    "cubemap": ["5"],
}


def run(program, kind, mode, a, b):
    p = subprocess.run([program, kind, mode, "%r" % a, "%r" % b] + CPP_CASES[kind] + ["%r" % v for v in POS], capture_output=True)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()
    return np.frombuffer(p.stdout, dtype=A.RAY)


def same_records(got, want):
    """the rule of the CLI comparisons: every record finite, at least 99 % of them equal bit for bit — both hosts work in
    double and round once, so a record differs only where a double lies within an ulp of a float32 rounding boundary"""
    assert got.shape == want.shape and np.array_equal(got["x"], want["x"]) and np.array_equal(got["y"], want["y"])
    assert np.isfinite(got["o"]).all() and np.isfinite(got["d"]).all()
    equal = (got.view(np.uint32).reshape(-1, 8) == want.view(np.uint32).reshape(-1, 8)).all(-1)
    assert equal.mean() >= 0.99
    assert np.abs(got["d"] - want["d"]).max() <= F32_EPS and np.abs(got["o"] - want["o"]).max() <= 4 * F32_EPS


@pytest.mark.parametrize("kind", sorted(CPP_CASES))
def test_cpp_generators_with_offsets_match(kind, program):
    gen, kw, _ = GENERATORS[kind]
    assert run(program, kind, "one", 0.0, 0.0).tobytes() == run(program, kind, "one", -0.0, 0.0).tobytes()
    same_records(run(program, kind, "one", 0.0, 0.0), gen(**kw))
    same_records(run(program, kind, "one", 0.3125, -0.4375), gen(offset=(0.3125, -0.4375), **kw))
    k = 5
    got = run(program, kind, "sets", k, 0)
    same_records(got, rays.ray_sets(gen, rt.Camera.sampleOffsets(k), **kw).reshape(-1))
